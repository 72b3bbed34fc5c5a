"""The recurrent update's whole-sequence strip kernels (csrc/lhw_mlp_strip.hip: lstm_seq_fwd_strip_kernel / lstm_seq_bwd_strip_kernel, the
two time loops of lhw_rnn_grad as one launch each) on the SIMT emulator, poison on: lhw_debug_lstm_seq with fused = 1 against fused = 0
(per step a thread-per-output fmaf-chain kernel and the two cell functions of csrc/lhw_lstm_cell.h).  Both run the same chains over
ascending k and the same cell arithmetic, so every output must be EQUAL: xh1, xh2 and the activated gates g1, g2 after the forward pass,
c1, c2, h2, and d loss / d pre-activation in g1, g2 after the backward pass.  tests/test_lstm_seq_gpu.py is the GPU twin."""
import ctypes

import numpy as np
import pytest

SENTINEL = 7.0
PAD_ROWS = 40          # rows behind every output that nobody may write (a ragged last slab has up to 31 dead rows)
FWD_OUT = ("xh1", "xh2", "g1", "g2", "c1", "c2", "h2")


def reset_flags(T, Bt):
    """[T][Bt] episode starts.  Column b takes pattern b % 4: only the t = 0 start; a start in the middle; starts at two consecutive steps;
    a start at t = T - 1.  A single column takes the last three together."""
    assert T >= 3
    r = np.zeros((T, Bt), np.uint8)
    r[0] = 1
    mid = (T - 1) // 2
    pat = {0: [], 1: [mid], 2: [mid, mid + 1], 3: [T - 1]}
    for b in range(Bt):
        for t in (pat[b % 4] if Bt > 1 else [mid, mid + 1, T - 1]):
            r[t, b] = 1
    return r


def has_all_patterns(r):
    T = r.shape[0]
    cols = [tuple(np.flatnonzero(r[:, b])) for b in range(r.shape[1])]
    only_first = any(c == (0,) for c in cols)
    middle = any(any(0 < t < T - 1 for t in c) for c in cols)
    consecutive = any(any(t + 1 in c for t in c if t > 0) for c in cols)
    at_last = any(T - 1 in c for c in cols)
    return only_first and middle and consecutive and at_last


def make_seq_case(H, Dp, T, Bt, O=12, seed=0):
    """Weights of one network's two cells (torch's uniform(-1/sqrt(H), 1/sqrt(H)) init, scaled up so the gates leave their linear range),
    inputs, reset flags and dh2 = dy Wout for a read-out of O outputs."""
    rs = np.random.default_rng(seed)
    f = np.float32
    K1, R = Dp + H, T * Bt
    u = lambda *s: (rs.uniform(-1, 1, size=s) * 2.0 / np.sqrt(H)).astype(f)
    c = dict(H=H, Dp=Dp, T=T, Bt=Bt, R=R, w1=u(4 * H, K1), bi1=u(4 * H), bh1=u(4 * H), w2=u(4 * H, 2 * H), bi2=u(4 * H), bh2=u(4 * H))
    c["x"] = rs.normal(size=(R, Dp)).astype(f)
    c["reset"] = reset_flags(T, Bt)
    dy, wo = rs.normal(size=(R, O)).astype(f), rs.normal(size=(O, H)).astype(f)
    c["dh2"] = (dy @ wo).astype(f)
    return c


def run_seq(L, c, fused, ptr=lambda a: a.ctypes.data, alloc=None, dev=lambda a: a, host=np.asarray, copy=lambda a: a.copy()):
    """Forward call, snapshot, backward call on sentinel-filled outputs.  `alloc(shape, dtype, fill)` / `ptr` / `dev` (host array -> the array
    the kernel reads) / `host` / `copy` let the GPU twin run the same steps on device buffers.  Returns host arrays: the seven forward outputs
    and `dg1`, `dg2` (g1, g2 after the backward pass), each with its PAD_ROWS guard rows."""
    from learninghumanoidwalking_amd._lib import LhwLstmSeqArgs
    alloc = alloc or (lambda shape, dt, fill: np.full(shape, fill, dt))
    H, Dp, T, Bt, R = c["H"], c["Dp"], c["T"], c["Bt"], c["R"]
    f = np.float32
    width = dict(xh1=Dp + H, xh2=2 * H, g1=4 * H, g2=4 * H, c1=H, c2=H, h2=H)
    xh1 = np.full((R + PAD_ROWS, Dp + H), SENTINEL, f)
    xh1[:R, :Dp] = c["x"]
    out = {k: alloc((R + PAD_ROWS, w), f, SENTINEL) for k, w in width.items() if k != "xh1"}
    out["xh1"] = copy(dev(xh1))
    scratch = alloc(((Dp + 3 * H) * 4 * H + 5 * Bt * H,), f, SENTINEL)
    keep = {k: dev(c[k]) for k in ("w1", "bi1", "bh1", "w2", "bi2", "bh2", "reset", "dh2")}
    a = LhwLstmSeqArgs(H=H, Dp=Dp, T=T, Bt=Bt, passes=1, scratch=ptr(scratch), **{k: ptr(v) for k, v in keep.items()}, **{k: ptr(v) for k, v in out.items()})
    assert L.lhw_debug_lstm_seq(ctypes.byref(a), int(fused), None) == 0, L.lhw_last_error()
    res = {k: host(copy(out[k])) for k in FWD_OUT}
    a.passes = 2
    assert L.lhw_debug_lstm_seq(ctypes.byref(a), int(fused), None) == 0, L.lhw_last_error()
    res["dg1"], res["dg2"] = host(out["g1"]), host(out["g2"])
    for k in ("c1", "c2", "h2", "xh1", "xh2"):
        assert np.array_equal(host(out[k]), res[k]), f"{k}: the backward pass must not write it"
    return res


def check_equal(c, un, fu):
    R, Dp = c["R"], c["Dp"]
    for k in FWD_OUT + ("dg1", "dg2"):
        a, b = un[k], fu[k]
        assert np.isfinite(b[:R]).all(), k
        assert (b[:R] != SENTINEL).all(), f"{k}: entry never written"
        assert (b[R:] == SENTINEL).all(), f"{k}: rows beyond the minibatch must not be written"
        assert np.array_equal(a, b), f"{k}: max |diff| = {np.abs(a[:R] - b[:R]).max():.3e}"
    assert np.array_equal(fu["xh1"][:R, :Dp], c["x"])
    # the recurrent slots are zero exactly where a step starts an episode (and hold the previous h elsewhere); the passes do something
    starts = c["reset"].reshape(-1).astype(bool)
    assert (fu["xh1"][:R, Dp:][starts] == 0).all() and (fu["xh2"][:R, c["H"]:][starts] == 0).all()
    assert (np.abs(fu["xh1"][:R, Dp:][~starts]).max(axis=1) > 0).all()
    assert np.abs(fu["dg1"][:R]).max() > 0 and np.abs(fu["dg2"][:R]).max() > 0


# H = 32 (one wave per workgroup), Bt = 1: one ragged slab; Bt = 33: two slabs, the second with one live row.  H = 64 (two waves), T = 4, for the
# widths of the actor's and the critic's read-out behind dh2
CASES = [
    pytest.param(dict(H=32, Dp=40, T=5, Bt=1), id="h32-bt1"),
    pytest.param(dict(H=32, Dp=40, T=5, Bt=33), id="h32-bt33"),
    pytest.param(dict(H=64, Dp=40, T=4, Bt=6, O=12), id="h64-bt6-actor"),
    pytest.param(dict(H=64, Dp=40, T=4, Bt=6, O=1), id="h64-bt6-critic"),
]


@pytest.mark.parametrize("kw", CASES)
def test_fused_lstm_sequence_equals_the_launch_per_step_reference_on_the_emulator(kw):
    from tests import emu
    L = emu.lib()
    c = make_seq_case(seed=5, **kw)
    if kw["Bt"] >= 4:
        assert has_all_patterns(c["reset"])
    else:
        r = c["reset"][:, 0]
        assert r[2] and r[3] and r[-1] and not r[1]
    un = run_seq(L, c, fused=0)
    fu = run_seq(L, c, fused=1)
    check_equal(c, un, fu)


def test_reset_patterns_are_what_the_cases_claim():
    r = reset_flags(5, 33)
    assert has_all_patterns(r) and has_all_patterns(reset_flags(4, 6))
    assert not has_all_patterns(np.ones((5, 4), np.uint8)) and not has_all_patterns(r[:, :1])


def test_lstm_sequence_strips_refuse_what_they_cannot_hold():
    from learninghumanoidwalking_amd._lib import LhwLstmSeqArgs
    from tests import emu
    L = emu.lib()
    z = np.zeros(64, np.float32)
    for H, Dp in ((48, 40), (288, 40), (64, 132)):
        a = LhwLstmSeqArgs(H=H, Dp=Dp, T=1, Bt=1, passes=3,
                           **{k: z.ctypes.data for k in ("w1", "bi1", "bh1", "w2", "bi2", "bh2", "reset", "dh2", "xh1", "xh2", "g1", "g2", "c1", "c2", "h2", "scratch")})
        assert L.lhw_debug_lstm_seq(ctypes.byref(a), 1, None) == -4      # LHW_ERR_UNSUPPORTED
