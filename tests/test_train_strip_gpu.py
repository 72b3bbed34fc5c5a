"""The update's train strip kernel on the chip: the comparisons of tests/test_emu_train_strip.py (fused launch == forward strip + head kernel
+ backward strip, bit for bit), and lhw_ppo_grad / lhw_ppo_apply / lhw_ppo_step with the fused path switched on and off on ONE handle
(lhw_ppo_debug_set_strip_fused): equal flat gradients, statistics and weights."""
import numpy as np
import pytest
import torch

from tests.test_emu_train_strip import CASES, check_equal, make_train_case, run_train_strip
from tests.test_optimizer_gpu import PAD_A, PAD_D, PAD_MIR_ACT, PAD_MIR_OBS, _ppo_batch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kw", CASES + [pytest.param(dict(B=1000, Dp=40, critic=False, twin0=1024), id="actor-mirror-1000-of-1024")])
def test_fused_train_strip_equals_the_three_launches(kw):
    from learninghumanoidwalking_amd import _lib
    L = _lib.lib()
    c = make_train_case(seed=3, **kw)
    dt = {np.dtype(np.float32): torch.float32, np.dtype(np.int32): torch.int32}
    alloc = lambda shape, t, fill: torch.full(shape, fill, dtype=dt[np.dtype(t)], device="cuda")
    args = dict(ptr=lambda t: t.data_ptr(), alloc=alloc, dev=lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda())
    un = run_train_strip(L, c, fused=0, **args)
    fu = run_train_strip(L, c, fused=1, **args)
    torch.cuda.synchronize()
    check_equal(c, un, fu, host=lambda t: t.cpu().numpy())


def _handle(mirror, learn_std, max_rows):
    from learninghumanoidwalking_amd.ppo_kernels import PpoKernels, reference_init
    from oracle import ppo_oracle as po
    kw = dict(mirror_obs=po.mirror_tables(PAD_MIR_OBS), mirror_act=po.mirror_tables(PAD_MIR_ACT)) if mirror else {}
    k = PpoKernels(PAD_D, PAD_A, hidden=256, max_rows=max_rows, learn_std=learn_std, entropy_coeff=0.01 if learn_std else 0.0, lr=1e-3, **kw)
    k.set_tensors(reference_init(PAD_D, PAD_A, 256, 0.223, generator_seed=7))
    return k


def _set_fused(k, on):
    from learninghumanoidwalking_amd import _lib
    _lib.check(k._L.lhw_ppo_debug_set_strip_fused(k._h, int(on)))


@pytest.mark.parametrize("B,R", [(256, 256), (200, 256), (33, 64)])
@pytest.mark.parametrize("learn_std", [False, True])
@pytest.mark.parametrize("mirror", [False, True])
def test_ppo_grad_and_apply_are_the_same_bits_with_the_fused_path_on_and_off(mirror, learn_std, B, R):
    """B == R (the mirrored rows follow without a gap), B < R (they start at R), a ragged twin slab (B = 33)."""
    k = _handle(mirror, learn_std, R)
    rs = np.random.default_rng(B + 2 * mirror + learn_std)
    k.set_obs_norm(rs.normal(size=PAD_D).astype(np.float32) * 0.1, (0.5 + rs.uniform(size=PAD_D)).astype(np.float32))
    xn, xm, act, logp, adv, ret, idx = _ppo_batch(k, rs, 512, 1, B)
    logp = logp + torch.tensor(rs.uniform(-0.5, 0.5, size=512).astype(np.float32)).cuda()      # ratios on both sides of the clip range
    theta0, res = k.theta.clone(), {}
    for on in (0, 1):
        _set_fused(k, on)
        k.theta.copy_(theta0)
        for t in (k.grad, k.adam_m, k.adam_v, k.stats):
            t.zero_()
        k.adam_step = 0
        k.grad_minibatch(xn, xm if mirror else None, act, logp, adv, ret, idx[0])
        torch.cuda.synchronize()
        assert k._L.lhw_ppo_debug_last_grad_fused(k._h) == on, "the path the switch asks for is the path that ran"
        grad, stats = k.grad.clone(), k.stats.clone()
        k.apply()
        torch.cuda.synchronize()
        res[on] = (grad, stats, k.theta.clone())
    assert res[0][0].abs().sum() > 0 and 0 < float(res[0][1][4]) < 1, "clip fraction strictly between 0 and 1"
    assert torch.equal(res[0][0], res[1][0]), "flat gradient"
    assert torch.equal(res[0][1], res[1][1]), "loss statistics"
    assert torch.equal(res[0][2], res[1][2]) and not torch.equal(res[1][2], theta0), "weights after lhw_ppo_apply"


@pytest.mark.parametrize("mirror", [False, True])
def test_two_graph_steps_equal_the_two_call_path(mirror, monkeypatch):
    """lhw_ppo_step (the captured graph, fused path on) twice == lhw_ppo_grad + lhw_ppo_apply twice with the fused path off."""
    monkeypatch.delenv("LHW_PPO_GRAPH", raising=False)
    B = 256
    graph, eager = _handle(mirror, True, B), _handle(mirror, True, B)
    _set_fused(graph, 1)
    _set_fused(eager, 0)
    rs = np.random.default_rng(11 + mirror)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        xn, xm, act, logp, adv, ret, idx = _ppo_batch(graph, rs, 1024, 2, B)
        xm = xm if mirror else None
        for t in range(2):
            graph.step_minibatch(xn, xm, act, logp, adv, ret, idx[t])
            eager.grad_minibatch(xn, xm, act, logp, adv, ret, idx[t])
            eager.apply()
        stream.synchronize()
    assert graph._L.lhw_ppo_debug_last_grad_fused(graph._h) == 1 and eager._L.lhw_ppo_debug_last_grad_fused(eager._h) == 0
    for name in ("theta", "adam_m", "adam_v"):
        assert torch.equal(getattr(graph, name), getattr(eager, name)), name
    assert torch.equal(graph.stats[:6], eager.stats[:6])
