"""Eval video: the host side of lhw_jpeg_encode (include/lhw.h) and a Motion-JPEG AVI writer.

The reference's eval appends every frame to an imageio video writer (rl/utils/eval.py:25-34, 63).  Here the frames the ray caster drew
(render.py) are coded as baseline JPEGs on the device -- colour conversion, DCT, quantisation and Huffman coding are the kernel's, as
include/lhw.h specifies them -- and only the compressed bytes cross to the host, which wraps every segment in the JFIF headers and the
frames in a RIFF AVI (`MJPG`: one complete JPEG per frame, no inter-frame coding, no audio).  No encoder library is involved.
"""
from __future__ import annotations

import ctypes
import struct

import numpy as np
import torch

from . import _lib

CHUNK_BYTES = 64 << 20      # encode() works in frame chunks whose scratch and output buffers each stay below this
MAX_CHUNK_FRAMES = 1024

# ITU-T T.81 Annex K.1 / K.2: the example quantisation tables, natural order
_Q_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
           18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
_Q_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
# Annex K.3 - K.6: BITS and HUFFVAL of the tables the kernel codes with (csrc/lhw_video.hip holds the same), as the DHT segments carry them
_DC_BITS = (bytes([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]), bytes([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]))
_AC_BITS = (bytes([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D]), bytes([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]))
_AC_VALS = (bytes.fromhex("01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a"
                          "434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9"
                          "aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"),
            bytes.fromhex("000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a3536373839"
                          "3a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7"
                          "a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"))
_ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
           35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)


def quant_tables(quality):
    """(luminance, chrominance) quantisation tables, 64 ints each in natural order: the Annex K tables under the usual quality scaling
    (1..100; 50 = the tables themselves, above it scale = 200 - 2 q per cent, below it 5000 / q), every entry clamped to 1..255."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"JPEG quality {quality!r} is not in 1..100")
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple([min(255, max(1, (t * scale + 50) // 100)) for t in table] for table in (_Q_LUMA, _Q_CHROMA))


def _segment(marker, payload):
    return bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + payload


def jfif_headers(width, height, qluma, qchroma):
    """Everything of a baseline JFIF file in front of lhw_jpeg_encode's segment: SOI, APP0, two DQT, SOF0 (Y 2x2, Cb, Cr), four DHT, DRI
    (one MCU row), SOS."""
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0" + struct.pack(">BBBHHBB", 1, 1, 0, 1, 1, 0, 0))
    for k, table in enumerate((qluma, qchroma)):
        out += _segment(0xDB, bytes([k]) + bytes(table[i] for i in _ZIGZAG))
    out += _segment(0xC0, struct.pack(">BHHB", 8, height, width, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for k in range(2):
        out += _segment(0xC4, bytes([k]) + _DC_BITS[k] + bytes(range(12)))
        out += _segment(0xC4, bytes([0x10 | k]) + _AC_BITS[k] + _AC_VALS[k])
    out += _segment(0xDD, struct.pack(">H", (width + 15) // 16))
    return out + _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


class JpegEncoder:
    """Baseline JPEGs of frames on `device`, coded by lhw_jpeg_encode.

    `library`: a ctypes handle of another build of the C ABI that _lib.declare was applied to (None: the GPU library); only with one may
    `device` be a CPU device."""

    def __init__(self, width, height, quality=90, device: int | torch.device = 0, library=None):
        if library is None and not torch.cuda.is_available():
            raise _lib.LhwError(-5, "no GPU visible: the JPEG encoder has no CPU fallback")
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if library is None and self.device.type != "cuda":
            raise _lib.LhwError(-5, f"device {self.device}: the JPEG encoder has no CPU fallback")
        self._L = _lib.lib() if library is None else library
        if getattr(self._L, "lhw_jpeg_encode", None) is None:
            raise _lib.LhwError(-4, "this build of the library does not export lhw_jpeg_encode")
        self.width, self.height, self.quality = int(width), int(height), int(quality)
        self.qluma, self.qchroma = quant_tables(quality)
        s = self.settings = _lib.LhwJpegSettings()
        s.width, s.height = self.width, self.height
        for i in range(64):
            s.qtable[0][i], s.qtable[1][i] = self.qluma[i], self.qchroma[i]
        self._frame_bytes = int(self._L.lhw_jpeg_scratch_bytes(ctypes.byref(s), 1))
        if self._frame_bytes < 0:
            _lib.check(-1, self._L)
        self.header = jfif_headers(self.width, self.height, self.qluma, self.qchroma)

    @property
    def frames_per_chunk(self) -> int:
        return max(1, min(MAX_CHUNK_FRAMES, CHUNK_BYTES // self._frame_bytes))

    def encode_segments(self, rgb):
        """One lhw_jpeg_encode call on the current stream for the uint8 tensor rgb [F][H][W][3] on the encoder's device: (segments, offsets)
        -- a uint8 device tensor holding the F entropy-coded segments back to back, and the int64 device tensor [F + 1] of their bounds."""
        if rgb.dtype != torch.uint8 or rgb.dim() != 4 or tuple(rgb.shape[1:]) != (self.height, self.width, 3) or rgb.device != self.device:
            raise ValueError(f"encode takes a uint8 tensor [F][{self.height}][{self.width}][3] on {self.device}, got {rgb.dtype} {tuple(rgb.shape)} on {rgb.device}")
        rgb = rgb.contiguous()
        F = rgb.shape[0]
        s = ctypes.byref(self.settings)
        need_scratch, need_out = int(self._L.lhw_jpeg_scratch_bytes(s, F)), int(self._L.lhw_jpeg_out_bytes(s, F))
        scratch = _lib.empty((need_scratch + 7) // 8, dtype=torch.int64, device=self.device)
        out = _lib.empty(max(need_out, 1), dtype=torch.uint8, device=self.device)
        offsets = torch.zeros(F + 1, dtype=torch.int64, device=self.device)
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream) if self.device.type == "cuda" else None
        _lib.check(self._L.lhw_jpeg_encode(s, F, ctypes.c_void_p(rgb.data_ptr()), ctypes.c_void_p(scratch.data_ptr()), need_scratch,
                                           ctypes.c_void_p(out.data_ptr()), need_out, ctypes.c_void_p(offsets.data_ptr()), stream), self._L)
        return out, offsets

    def encode(self, rgb):
        """Complete JFIF files, a list of F byte strings, of the frames rgb [F][H][W][3] (what Renderer.render returns).  Frames are coded in
        chunks of frames_per_chunk; of every chunk only the offsets and the compressed bytes are copied to the host."""
        files = []
        for f0 in range(0, rgb.shape[0], self.frames_per_chunk):
            out, offsets = self.encode_segments(rgb[f0:f0 + self.frames_per_chunk])
            off = offsets.cpu().numpy()
            data = out[:int(off[-1])].cpu().numpy().tobytes()
            files += [self.header + data[off[k]:off[k + 1]] + b"\xff\xd9" for k in range(len(off) - 1)]
        return files


class MjpegWriter:
    """A RIFF AVI file of JPEG frames (`MJPG`): hdrl (avih, one strl: vids / MJPG with a BITMAPINFOHEADER), movi of `00dc` chunks padded to
    even length, idx1.  Sizes and frame counts are patched on close().  A context manager."""

    _HDRL = 4 + (8 + 56) + (12 + (8 + 56) + (8 + 40))      # 'hdrl' + avih chunk + LIST strl (strh chunk, strf chunk)

    def __init__(self, path, width, height, fps):
        if not (width >= 1 and height >= 1 and fps > 0):
            raise ValueError(f"MjpegWriter: size {width} x {height}, fps {fps}")
        self.width, self.height, self.fps = int(width), int(height), float(fps)
        self._index, self._largest = [], 0
        self._f = open(path, "wb")
        self._f.write(self._header(0, 0))
        self._movi = self._f.tell() - 4      # the position of 'movi': idx1 offsets count from here

    def _header(self, frames, movi_bytes):
        rate, scale = int(round(self.fps * 1000)), 1000
        usec = int(round(1e6 / self.fps))
        avih = struct.pack("<14I", usec, int(self._largest * self.fps), 0, 0x10, frames, 0, 1, self._largest, self.width, self.height, 0, 0, 0, 0)
        strh = b"vids" + b"MJPG" + struct.pack("<IHHIIIIIIII4H", 0, 0, 0, 0, scale, rate, 0, frames, self._largest, 0xFFFFFFFF, 0, 0, 0, self.width, self.height)
        strf = struct.pack("<IiiHH4sIiiII", 40, self.width, self.height, 1, 24, b"MJPG", self.width * self.height * 3, 0, 0, 0, 0)
        hdrl = b"LIST" + struct.pack("<I", self._HDRL) + b"hdrl" + b"avih" + struct.pack("<I", 56) + avih + \
            b"LIST" + struct.pack("<I", 4 + 8 + 56 + 8 + 40) + b"strl" + b"strh" + struct.pack("<I", 56) + strh + b"strf" + struct.pack("<I", 40) + strf
        riff = 4 + len(hdrl) + 8 + 4 + movi_bytes + 8 + 16 * frames
        return b"RIFF" + struct.pack("<I", riff) + b"AVI " + hdrl + b"LIST" + struct.pack("<I", 4 + movi_bytes) + b"movi"

    def add(self, jpeg_bytes):
        """append one frame: a complete JPEG file"""
        data = bytes(jpeg_bytes)
        self._index.append((self._f.tell() - self._movi, len(data)))
        self._largest = max(self._largest, len(data))
        self._f.write(b"00dc" + struct.pack("<I", len(data)) + data + b"\0" * (len(data) & 1))

    @property
    def frames(self) -> int:
        return len(self._index)

    def close(self):
        if self._f is None:
            return
        movi_bytes = self._f.tell() - self._movi - 4
        self._f.write(b"idx1" + struct.pack("<I", 16 * len(self._index)) + b"".join(b"00dc" + struct.pack("<III", 0x10, o, n) for o, n in self._index))
        self._f.seek(0)
        self._f.write(self._header(len(self._index), movi_bytes))
        self._f.close()
        self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
