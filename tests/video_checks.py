"""TEST INFRASTRUCTURE: the cases of lhw_jpeg_encode shared by tests/test_video.py (the emulated build) and tests/test_video_gpu.py (the GPU
library).  Every case names the smallest image at which its code path exists; every frame's entropy-coded segment must equal
tests/jpeg_oracle.py's byte for byte, and every buffer the call writes carries 64 guard bytes that must come back untouched.

`make(width, height, quality)` returns the JpegEncoder under test (its device decides where the tensors live).
"""
import ctypes
import functools

import numpy as np
import torch

from tests import jpeg_oracle as O

GUARD = 64


def _noise(seed, F, H, W):
    return np.random.default_rng(seed).integers(0, 256, size=(F, H, W, 3), dtype=np.uint8)


def _squares():      # 32 x 16: a black and a white 16 x 16 square
    a = np.zeros((1, 16, 32, 3), dtype=np.uint8)
    a[:, :, 16:] = 255
    return a


def _checkerboard(lo=0, hi=255):      # 16 x 16, one-pixel squares
    yy, xx = np.mgrid[0:16, 0:16]
    return np.repeat((lo + ((xx + yy) & 1) * (hi - lo)).astype(np.uint8)[None, :, :, None], 3, axis=3)


def _smooth(F, H, W):      # three different gradients with a little noise: mid-size coefficients, some zero runs
    yy, xx = np.mgrid[0:H, 0:W]
    frames = [np.stack([(9 * xx + 3 * yy + 40 * f) % 256, (5 * yy + 70 * f) % 256, (4 * xx * (f + 1) + 7 * yy) % 256], axis=2) for f in range(F)]
    return ((np.stack(frames) + _noise(7, F, H, W) % 8) % 256).astype(np.uint8)


# name -> (frames uint8 [F][H][W][3], the qualities the case runs at)
CASES = {
    "1x1": (lambda: _noise(1, 1, 1, 1), (100, 50)),                       # less than one MCU: the one pixel replicated both ways
    "8x8": (lambda: _noise(2, 1, 8, 8), (100, 50)),                       # one Y block of pixels, three of replicated edges
    "flat16": (lambda: np.full((1, 16, 16, 3), (200, 90, 30), dtype=np.uint8), (100, 50)),      # one MCU, every AC zero: EOB only
    "24x20": (lambda: _smooth(1, 20, 24), (100, 50)),                     # 2 x 2 MCUs clipped on both edges, one restart marker
    "noise16x176": (lambda: _noise(3, 1, 176, 16), (100, 50)),            # eleven MCU rows: RST0 and RST1 twice, stuffed FF 00
    "squares32x16": (_squares, (100,)),                                   # DC differences of the largest category
    "checker16": (_checkerboard, (100, 50)),                              # the largest AC category, coefficient 63 (no EOB)
    # (at quality 50 the full-contrast checkerboard keeps a non-zero coefficient on every odd anti-diagonal: its longest zero run is 9.  The
    # low-contrast one keeps coefficient 63 alone, behind 62 zeros: three ZRL codes and no EOB)
    "checker16_soft": (lambda: _checkerboard(112, 144), (50,)),
    "three24x20": (lambda: _smooth(3, 20, 24), (100, 50)),                # frame_offset_dev and the compaction
    # 25 MCUs = 150 blocks in the row: three passes of 64 lanes, so left-over bits and DC predictions cross from pass to pass
    "wide400x8": (lambda: _noise(4, 1, 8, 400), (100, 50)),
}
CASE_IDS = [(n, q) for n, (_, qs) in CASES.items() for q in qs]


@functools.lru_cache(maxsize=None)
def frames(name):
    a = CASES[name][0]()
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def oracle(name, quality):
    """[(blocks, segment)] per frame, computed once"""
    ql, qc = O.quant_tables(quality)
    return [O.encode(f, ql, qc) for f in frames(name)]


def _max_zero_run(block, zz):
    """the longest run of zeros in front of a non-zero AC coefficient"""
    best = run = 0
    for k in range(1, 64):
        if block[zz[k]] == 0:
            run += 1
        else:
            best, run = max(best, run), 0
    return best


def check_properties(name, quality):
    """that the case's image takes the code path it is there for, read off the oracle's output"""
    out = oracle(name, quality)
    blocks, seg = out[0]
    flat = blocks.reshape(-1, 64)
    if name == "flat16":
        assert not flat[:, 1:].any()
    if name == "24x20":
        assert blocks.shape[:2] == (2, 2) and seg.count(b"\xff\xd0") == 1
    if name == "noise16x176":
        assert blocks.shape[0] == 11 and b"\xff\x00" in seg
        assert [m for m in range(8) if seg.count(bytes([0xFF, 0xD0 + m])) == 2] == [0, 1]
    if name == "squares32x16":
        ydc = blocks[0, :, :4, 0].reshape(-1)
        assert max(abs(int(d)).bit_length() for d in np.diff(ydc)) == 11
    if name == "checker16" and quality == 100:
        assert max(abs(int(c)).bit_length() for c in flat[:, 1:].reshape(-1)) == 10 and flat[:4, 63].all()
    if name == "checker16_soft":
        assert max(_max_zero_run(b, O.zigzag_order()) for b in flat) == 62 and flat[:4, 63].all()
    if name == "three24x20":
        assert len({s for _, s in out}) == 3


def encode_guarded(enc, rgb):
    """lhw_jpeg_encode of the tensor rgb [F][H][W][3] with guard bytes behind scratch, output and offsets: the F segments as bytes"""
    L, s, F, dev = enc._L, ctypes.byref(enc.settings), rgb.shape[0], rgb.device
    need_scratch, need_out = L.lhw_jpeg_scratch_bytes(s, F), L.lhw_jpeg_out_bytes(s, F)
    sizes = (need_scratch, need_out, 8 * (F + 1))
    scratch, out, off = (torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device=dev) for n in sizes)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if dev.type == "cuda" else None
    rc = L.lhw_jpeg_encode(s, F, ctypes.c_void_p(rgb.data_ptr()), ctypes.c_void_p(scratch.data_ptr()), need_scratch, ctypes.c_void_p(out.data_ptr()),
                           need_out, ctypes.c_void_p(off.data_ptr()), stream)
    assert rc == 0, L.lhw_last_error()
    for buf, n in zip((scratch, out, off), sizes):
        assert (buf[n:] == 0xA5).all()
    bounds = off[:8 * (F + 1)].cpu().numpy().view(np.int64)
    data = out.cpu().numpy().tobytes()
    assert bounds[0] == 0 and (np.diff(bounds) > 0).all() and bounds[-1] <= need_out
    return [data[bounds[f]:bounds[f + 1]] for f in range(F)]


def check_case(make, name, quality):
    """The case through the encoder under test, against the oracle; returns the complete JFIF files JpegEncoder.encode gives."""
    check_properties(name, quality)
    a = frames(name)
    enc = make(a.shape[2], a.shape[1], quality)
    assert (enc.qluma, enc.qchroma) == O.quant_tables(quality)
    rgb = torch.from_numpy(a.copy()).to(enc.device)
    want = [seg for _, seg in oracle(name, quality)]
    got = encode_guarded(enc, rgb)
    for f, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name} q{quality} frame {f}: {len(g)} bytes against the oracle's {len(w)}, first difference at byte " \
                       f"{next((i for i, (x, y) in enumerate(zip(g, w)) if x != y), min(len(g), len(w)))}"
    files = enc.encode(rgb)
    assert files == [enc.header + w + b"\xff\xd9" for w in want]
    return files
