"""The update's train strip kernel (csrc/lhw_mlp_strip.hip: forward layers, PPO head and backward layers of one network on slabs that
stay in LDS) on the SIMT emulator, poison on: lhw_debug_mlp_train_strip with fused = 1 against fused = 0 (forward strip, the head
function as a thread-per-row kernel, backward strip).  Both run the same per-row fmaf chains and the same head function, so every
output must be EQUAL: h1, h2, y, dy, dh2, dh1, the dstd rows and the rows' loss terms (whose sums are the step's statistics).
tests/test_train_strip_gpu.py is the GPU twin."""
import ctypes

import numpy as np
import pytest

from tests.test_emu_mlp_strip import make_case, reference

CLIP = 0.2
OUTPUTS = ("h1", "h2", "y", "dy", "dh2", "dh1", "dstd", "stat_rows")


def make_train_case(B, Dp, critic, twin0=0, seed=0):
    """Weights and a minibatch of B rows (rows [twin0, twin0 + B) of x: the mirrored twins).  old_logp is the log-density under the
    float64 forward pass shifted by up to +-0.5, so the PPO ratio exp(-shift) leaves the clip range on both sides; advantages of both
    signs: every branch of the head runs."""
    O, Op = (1, 4) if critic else (12, 16)
    rows = twin0 + B if twin0 else B
    c = make_case(R=rows, Dp=Dp, O=O, Op=Op, seed=seed)
    rs = np.random.default_rng(1000 + seed)
    f = np.float32
    c.update(B=B, twin0=twin0, critic=critic, rows=rows)
    c["ret"] = rs.normal(size=B).astype(f)
    if critic:
        return c
    if twin0:
        c["x"][B:twin0] = np.nan                         # rows between the two halves belong to nobody
    mu = reference(c)[2][:B, :O]
    stdv = rs.uniform(0.15, 0.4, size=O)
    act = mu + stdv * rs.normal(size=(B, O))
    logp = (-0.5 * ((act - mu) / stdv) ** 2 - np.log(stdv) - 0.9189385332046727).sum(1)
    shift = rs.uniform(-0.5, 0.5, size=B)
    c.update(act=act.astype(f), stdv=stdv.astype(f), old_logp=(logp + shift).astype(f), adv=rs.normal(size=B).astype(f), shift=shift,
             act_src=rs.permutation(O).astype(np.int32), act_sign=rs.choice([-1.0, 1.0], size=O).astype(f))
    ratio = np.exp(-shift)
    assert (ratio > 1 + CLIP + 0.05).any() and (ratio < 1 - CLIP - 0.05).any() and (np.abs(ratio - 1) < CLIP - 0.05).any()
    assert (c["adv"] < 0).any() and (c["adv"] > 0).any()
    return c


def run_train_strip(L, c, fused, ptr=lambda a: a.ctypes.data, alloc=None, dev=lambda a: a):
    """One lhw_debug_mlp_train_strip call on sentinel-filled outputs.  `alloc(shape, dtype, fill)` / `ptr` / `dev` (host array -> the
    array the kernel reads) let the GPU twin run the same steps on device buffers."""
    from learninghumanoidwalking_amd._lib import LhwTrainStripArgs
    alloc = alloc or (lambda shape, dt, fill: np.full(shape, fill, dt))
    rows, B, H, Op = c["rows"], c["B"], c["H"], c["Op"]
    f = np.float32
    out = dict(h1=alloc((rows, H), f, 7.0), h2=alloc((rows, H), f, 7.0), y=alloc((rows, Op), f, 7.0), dy=alloc((rows, Op), f, 7.0),
               dh2=alloc((rows, H), f, 7.0), dh1=alloc((rows, H), f, 7.0), dstd=alloc((B, Op), f, 7.0), stat_rows=alloc((6, B + 5), f, 7.0))
    wt = alloc(((c["Dp"] + 256 + Op) * 256,), f, 0)
    keep = {k: dev(c[k]) for k in ("w1", "b1", "w2", "b2", "w3", "b3", "x", "ret", "act", "old_logp", "adv", "stdv", "act_src", "act_sign") if k in c}
    a = LhwTrainStripArgs(H=H, Dp=c["Dp"], O=c["O"], Op=Op, ldx=c["Dp"], B=B, twin0=c["twin0"], critic=int(c["critic"]), clip=CLIP, mirror_coeff=0.4,
                          stat_ld=B + 5, wt_scratch=ptr(wt), **{k: ptr(v) for k, v in keep.items()}, **{k: ptr(v) for k, v in out.items()})
    assert L.lhw_debug_mlp_train_strip(ctypes.byref(a), int(fused), None) == 0
    return out


def check_equal(c, un, fu, host=np.asarray):
    """fused == unfused on every output; rows nobody owns keep the sentinel; live rows are finite; statistics (the sums of the rows'
    terms) within 1e-6 relative."""
    B, twin0, rows = c["B"], c["twin0"], c["rows"]
    live = np.zeros(rows, bool)
    live[:B] = True
    if twin0:
        live[twin0:twin0 + B] = True
    for k in OUTPUTS:
        if c["critic"] and k == "dstd":
            continue
        a, b = host(un[k]), host(fu[k])
        assert np.array_equal(a, b, equal_nan=True), k
        if k not in ("dstd", "stat_rows"):
            assert np.isfinite(b[live]).all(), k
            assert (b[~live] == 7.0).all(), f"{k}: rows beyond the minibatch must not be written"
    terms = [1] if c["critic"] else [0, 2, 3, 4, 5]
    su, sf = host(un["stat_rows"]).astype(np.float64), host(fu["stat_rows"]).astype(np.float64)
    for k in range(6):
        if k in terms:
            assert np.isfinite(sf[k, :B]).all() and (sf[k, B:] == 7.0).all()
            np.testing.assert_allclose(sf[k, :B].sum(), su[k, :B].sum(), rtol=1e-6, atol=0)
        else:
            assert (sf[k] == 7.0).all()
    if not c["critic"]:
        d = host(fu["dstd"])
        assert np.isfinite(d).all() and (d[:, c["O"]:] == 0).all()
        cf = host(fu["stat_rows"])[4, :B]
        assert (cf == 1).any() and (cf == 0).any(), "rows inside and outside the clip range"
        if twin0:
            assert (host(fu["stat_rows"])[2, :B] > 0).all(), "mirror term"
            assert np.abs(host(fu["dy"])[twin0:twin0 + B]).max() > 0


# B = 64: one slab; 96 / 33: a ragged last slab (with twins: a ragged twin slab, dead rows in both tiles); 128 rows with the twins starting at
# R = 160 > B; Dp = 40 and 64 (the input slab's capacity); the critic's single output
CASES = [
    pytest.param(dict(B=64, Dp=40, critic=False), id="actor-64"),
    pytest.param(dict(B=96, Dp=64, critic=False), id="actor-96-dp64"),
    pytest.param(dict(B=33, Dp=40, critic=False), id="actor-33"),
    pytest.param(dict(B=128, Dp=40, critic=False, twin0=160), id="actor-mirror-128-of-160"),
    pytest.param(dict(B=33, Dp=64, critic=False, twin0=33), id="actor-mirror-33-dp64"),
    pytest.param(dict(B=96, Dp=40, critic=False, twin0=100), id="actor-mirror-96-of-100"),
    pytest.param(dict(B=64, Dp=40, critic=True), id="critic-64"),
    pytest.param(dict(B=96, Dp=64, critic=True), id="critic-96-dp64"),
    pytest.param(dict(B=33, Dp=40, critic=True), id="critic-33"),
]


@pytest.mark.parametrize("kw", CASES)
def test_fused_train_strip_equals_the_three_launches_on_the_emulator(kw):
    from tests import emu
    L = emu.lib()
    c = make_train_case(seed=3, **kw)
    un = run_train_strip(L, c, fused=0)
    fu = run_train_strip(L, c, fused=1)
    check_equal(c, un, fu)


def test_train_strip_refuses_what_it_cannot_hold():
    from tests import emu
    L = emu.lib()
    c = make_train_case(B=8, Dp=40, critic=True, seed=1)
    c["Op"] = 8                                             # the critic head is one value in rows of four
    from learninghumanoidwalking_amd._lib import LhwTrainStripArgs
    z = np.zeros(8, np.float32)
    a = LhwTrainStripArgs(H=256, Dp=40, O=1, Op=8, ldx=40, B=8, critic=1, stat_ld=8,
                          **{k: z.ctypes.data for k in ("w1", "b1", "w2", "b2", "w3", "b3", "x", "ret", "h1", "h2", "y", "dy", "dh2", "dh1", "stat_rows", "wt_scratch")})
    assert L.lhw_debug_mlp_train_strip(ctypes.byref(a), 1, None) != 0
