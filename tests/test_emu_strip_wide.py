"""The WIDE instantiations of the MLP strip kernels (csrc/lhw_mlp_strip.hip: padded input rows of 68 .. 256 columns, the rows of an
observation history) on the SIMT emulator, poison on.  Their arithmetic contract is the per-layer GEMM path they take over: every layer,
the read-out included, ONE fmaf chain over ascending k with the bias behind it.  So
  forward strip   y EQUAL to lhw_debug_policy_step's plain launch (the reference of the history rollout's in-wave step) on the same rows,
                  h1 / h2 / y within the float64 tolerances of tests/test_emu_mlp_strip.py, rows beyond R untouched, both workgroup shapes;
  train strip     fused = 1 EQUAL to fused = 0 on every output, where fused = 0 at these widths is independent code in the GEMM path's
                  order (a thread per output, plain chains);
  refusals        widths that are no multiple of 4 or beyond the slab.
tests/test_strip_wide_gpu.py is the GPU twin."""
import ctypes

import numpy as np
import pytest

from tests.test_emu_mlp_strip import _ptr, make_case, reference, run_forward
from tests.test_emu_train_strip import check_equal, make_train_case, run_train_strip

UNSUPPORTED = -4


def policy_step_reference(L, c, ptr=_ptr, alloc=None, dev=lambda a: a):
    """y [R][Op] of lhw_debug_policy_step's plain launch on c's rows: identity normalisation, deterministic.  `alloc` / `ptr` / `dev` as in
    tests/test_emu_train_strip.run_train_strip (the GPU twin runs the same steps on device buffers)."""
    from learninghumanoidwalking_amd._lib import LhwRolloutPolicy
    alloc = alloc or (lambda shape, dt, fill: np.full(shape, fill, dt))
    f = np.float32
    R, Dp, O, Op = c["R"], c["Dp"], c["O"], c["Op"]
    keep = dict(w1t=dev(np.ascontiguousarray(c["w1"].T)), b1=dev(c["b1"]), w2t=dev(np.ascontiguousarray(c["w2"].T)), b2=dev(c["b2"]),
                w3t=dev(np.ascontiguousarray(c["w3"].T)), b3=dev(c["b3"]), stdv=dev(np.full(O, 0.3, f)), obs_mean=dev(np.zeros(Dp, f)),
                obs_std=dev(np.ones(Dp, f)))
    x = dev(c["x"])
    view = LhwRolloutPolicy(obs_dim=Dp, obs_pad=Dp, act_dim=O, act_pad=Op, hidden=256, deterministic=1, fp16_operands=0, seed=1, counter=0,
                            **{k: ptr(v) for k, v in keep.items()})
    y, act, logp = alloc((R, Op), f, 7.0), alloc((R, O), f, 7.0), alloc((R,), f, 7.0)
    assert L.lhw_debug_policy_step(ctypes.byref(view), ptr(x), R, 0, 0, ptr(y), ptr(act), ptr(logp), None) == 0
    return y


FORWARD = [(Dp, R, O, Op) for Dp in (68, 128, 256) for R in (1, 37, 70) for O, Op in ((12, 16), (1, 4))]


@pytest.mark.parametrize("Dp,R,O,Op", FORWARD)
def test_wide_forward_strip_is_the_gemm_order_on_the_emulator(Dp, R, O, Op, monkeypatch):
    """68: the first width past the narrow slab, no multiple of the 16-k step; 256: the input fills the whole slab.  R = 1 / 37: a ragged slab;
    70: for the 64-row shape a full slab and a ragged one."""
    from tests import emu
    L = emu.lib()
    c = make_case(R=R, Dp=Dp, O=O, Op=Op, seed=Dp + R)
    outs = {}
    for shape in ("small", "big"):
        monkeypatch.setenv("LHW_DEBUG_STRIP_SHAPE", shape)
        outs[shape] = run_forward(L, c)
    yref = policy_step_reference(L, c)
    r1, r2, ry = reference(c)
    for shape, (h1, h2, y) in outs.items():
        assert (h1[R:] == 7.0).all() and (h2[R:] == 7.0).all() and (y[R:] == 7.0).all(), "rows beyond R must not be written"
        assert (y[:R, O:] == 7.0).all(), "pad columns of the read-out are left alone"
        np.testing.assert_array_equal(y[:R, :O], yref[:, :O], err_msg=shape)
        np.testing.assert_allclose(h1[:R], r1, rtol=0, atol=2e-5)
        np.testing.assert_allclose(h2[:R], r2, rtol=0, atol=5e-5)
        np.testing.assert_allclose(y[:R, :O], ry[:, :O], rtol=0, atol=5e-5)
    for a, b in zip(outs["small"], outs["big"]):
        np.testing.assert_array_equal(a, b)


# the twins: mirroring is refused for history envs, but the kernel text is shared with the narrow instantiation and must not break
TRAIN = [
    pytest.param(dict(B=33, Dp=68, critic=False), id="actor-33-dp68"),
    pytest.param(dict(B=96, Dp=68, critic=False), id="actor-96-dp68"),
    pytest.param(dict(B=33, Dp=256, critic=False), id="actor-33-dp256"),
    pytest.param(dict(B=96, Dp=256, critic=False), id="actor-96-dp256"),
    pytest.param(dict(B=33, Dp=128, critic=False, twin0=33), id="actor-mirror-33-dp128"),
    pytest.param(dict(B=33, Dp=128, critic=True), id="critic-33-dp128"),
    pytest.param(dict(B=96, Dp=128, critic=True), id="critic-96-dp128"),
]


@pytest.mark.parametrize("kw", TRAIN)
def test_wide_train_strip_equals_the_gemm_order_on_the_emulator(kw):
    from tests import emu
    L = emu.lib()
    c = make_train_case(seed=3, **kw)
    un = run_train_strip(L, c, fused=0)
    fu = run_train_strip(L, c, fused=1)
    check_equal(c, un, fu)


def test_narrow_train_strip_still_equals_its_three_launches():
    from tests import emu
    L = emu.lib()
    c = make_train_case(seed=3, B=96, Dp=64, critic=False)
    check_equal(c, run_train_strip(L, c, fused=0), run_train_strip(L, c, fused=1))


@pytest.mark.parametrize("Dp", [260, 66])
def test_widths_beyond_the_slab_or_off_the_16_byte_grid_are_refused(Dp):
    from learninghumanoidwalking_amd._lib import LhwTrainStripArgs
    from tests import emu
    L = emu.lib()
    c = make_case(R=8, Dp=Dp, O=12, Op=16, seed=1)
    f = np.float32
    h1, h2, y = np.full((8, 256), 7.0, f), np.full((8, 256), 7.0, f), np.full((8, 16), 7.0, f)
    wt = np.full((Dp + 256 + 16) * 256, 7.0, f)
    rc = L.lhw_debug_mlp_strip_forward(256, Dp, 12, 16, _ptr(c["w1"]), _ptr(c["b1"]), _ptr(c["w2"]), _ptr(c["b2"]), _ptr(c["w3"]), _ptr(c["b3"]),
                                       _ptr(c["x"]), Dp, 8, _ptr(h1), _ptr(h2), _ptr(y), _ptr(wt), None)
    assert rc == UNSUPPORTED
    out = {k: np.full((8, 256 if k in ("h1", "h2", "dh2", "dh1") else 16), 7.0, f) for k in ("h1", "h2", "y", "dy", "dh2", "dh1", "dstd", "stat_rows")}
    z = np.zeros(16, f)
    a = LhwTrainStripArgs(H=256, Dp=Dp, O=12, Op=16, ldx=Dp + (-Dp) % 4, B=8, critic=0, clip=0.2, stat_ld=16, wt_scratch=_ptr(wt),
                          **{k: _ptr(c[k]) for k in ("w1", "b1", "w2", "b2", "w3", "b3", "x")}, **{k: _ptr(z) for k in ("act", "old_logp", "adv", "stdv")},
                          **{k: _ptr(v) for k, v in out.items()})
    assert L.lhw_debug_mlp_train_strip(ctypes.byref(a), 1, None) == UNSUPPORTED
    assert L.lhw_debug_mlp_train_strip(ctypes.byref(a), 0, None) == UNSUPPORTED
    for v in (h1, h2, y, wt, *out.values()):
        assert (v == 7.0).all(), "a refused call writes nothing"
