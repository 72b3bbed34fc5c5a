"""The recurrent update's whole-sequence strip kernels on the chip: the comparisons of tests/test_emu_lstm_seq.py (one launch per pass ==
the launch-per-step reference, bit for bit), lhw_rnn_grad with the kernels switched on and off on ONE handle (lhw_rnn_debug_set_seq_fused):
equal flat gradients and statistics, and recurrent training under each setting of LHW_RNN_SEQ_FUSED: equal weights."""
import os

import numpy as np
import pytest
import torch

from tests.test_emu_lstm_seq import CASES, check_equal, make_seq_case, run_seq
from tests.test_rnn_gpu import G, MIR_ACT, MIR_OBS, NET, _args, _columns, _kernels

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kw", CASES + [pytest.param(dict(H=256, Dp=40, T=3, Bt=3), id="h256-bt3")])
def test_fused_lstm_sequence_equals_the_launch_per_step_reference(kw):
    from learninghumanoidwalking_amd import _lib
    L = _lib.lib()
    c = make_seq_case(seed=5, **kw)
    dt = {np.dtype(np.float32): torch.float32}
    alloc = lambda shape, t, fill: torch.full(shape, fill, dtype=dt[np.dtype(t)], device="cuda")
    args = dict(ptr=lambda t: t.data_ptr(), alloc=alloc, dev=lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda(),
                host=lambda t: t.cpu().numpy(), copy=lambda t: t.clone())
    un = run_seq(L, c, fused=0, **args)
    fu = run_seq(L, c, fused=1, **args)
    check_equal(c, un, fu)


def _grad_both_ways(k, call, expect_fused=1):
    """grad_columns under both switch settings on one handle -> {on: (flat grad, stats)}; asserts which path ran"""
    res = {}
    for on in (0, 1):
        k.set_seq_fused(on)
        k.grad.zero_()
        k.stats.zero_()
        call()
        torch.cuda.synchronize()
        assert k.last_grad_fused == (expect_fused if on else 0), "the path the switch asks for is the path that ran"
        res[on] = (k.grad.clone(), k.stats.clone())
    assert torch.isfinite(res[0][0]).all() and res[0][0].abs().sum() > 0
    return res


def test_fixture_gradient_is_the_same_bits_with_the_sequence_strips_on_and_off():
    """the inputs of the reference fixture rppo_h32_padded.npz (H = 32, no mirroring, episode starts inside the columns)"""
    g = np.load(os.path.join(G, "rppo_h32_padded.npz"))
    obs, reset, act, ret, adv, old_logp, done = _columns(g, 0)
    T, B = reset.shape
    k = _kernels(g, False, T, B)
    c = lambda x: x.cuda().contiguous()
    xn, xm = k.normalize(c(obs.reshape(T * B, -1)))
    cols = torch.arange(B, dtype=torch.int32, device="cuda")
    a = (c(act.reshape(T * B, -1)), c(old_logp.reshape(-1)), c(adv.reshape(-1)), c(ret.reshape(-1)), c(done), cols)
    res = _grad_both_ways(k, lambda: k.grad_columns(T, B, xn, xm, *a))
    assert torch.equal(res[0][0], res[1][0]), "flat gradient"
    assert torch.equal(res[0][1], res[1][1]), "loss statistics"


def _random_case(H, T, N, cols, mirror, learn_std=False):
    from learninghumanoidwalking_amd.rnn_kernels import RnnKernels
    from oracle import ppo_oracle as po
    rs = np.random.default_rng(17 + H + mirror)
    D, A = 37, 12
    kw = dict(mirror_obs=po.mirror_tables(MIR_OBS, [29, 30]), mirror_act=po.mirror_tables(MIR_ACT)) if mirror else {}
    k = RnnKernels(D, A, hidden=H, seq_len=T, seq_cols=len(cols), rollout_rows=N, learn_std=learn_std, **kw)
    gen = torch.Generator().manual_seed(3)
    shapes = [(4 * H, D), (4 * H, H), (4 * H,), (4 * H,), (4 * H, H), (4 * H, H), (4 * H,), (4 * H,)]
    for net, O in (("a", A), ("c", 1)):
        w = [torch.randn(*s, generator=gen) * 0.1 for s in shapes] + [torch.randn(O, H, generator=gen) * 0.05, torch.randn(O, generator=gen) * 0.01]
        k.set_tensors({f"{net}_{n}": t for n, t in zip(NET, w)})
    k.set_tensors({"stds": torch.full((A,), 0.223)})
    k.set_obs_norm(rs.normal(size=D).astype(np.float32) * 0.1, (0.5 + rs.uniform(size=D)).astype(np.float32))
    f = lambda *s: torch.tensor(rs.normal(size=s).astype(np.float32)).cuda()
    done = np.zeros((T, N), np.uint8)
    done[1, :] = 1          # every column: starts at t = 0 and t = 2 ...
    done[2, ::2] = 2        # ... and, every other one, at two consecutive steps
    done[T - 2, 1] = 1      # a start at t = T - 1
    xn, xm = k.normalize(f(T * N, D))
    act, logp = f(T * N, A) * 0.3, f(T * N) * 0.3 - 8.0
    a = (act, logp, f(T * N), f(T * N), torch.tensor(done).cuda(), torch.tensor(cols, dtype=torch.int32).cuda())
    return k, (lambda: k.grad_columns(T, N, xn, xm if mirror else None, *a))


@pytest.mark.parametrize("mirror", [False, True])
def test_h256_gradient_is_the_same_bits_with_the_sequence_strips_on_and_off(mirror):
    """H = 256 (eight waves per workgroup), T = 6, 3 of 5 columns in a shuffled order; with mirroring the twins are rows 3 .. 5 of each step"""
    k, call = _random_case(256, 6, 5, [4, 0, 2], mirror, learn_std=True)
    res = _grad_both_ways(k, call)
    assert torch.equal(res[0][0], res[1][0]), "flat gradient"
    assert torch.equal(res[0][1], res[1][1]), "loss statistics"


def test_a_hidden_width_outside_the_covered_set_keeps_the_launch_per_step_path():
    k, call = _random_case(48, 6, 5, [4, 0, 2], True)
    res = _grad_both_ways(k, call, expect_fused=0)
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_recurrent_training_gives_the_same_weights_under_each_switch_setting(tmp_path, monkeypatch):
    """two PPO iterations of jvrc_walk --recurrent (8 envs, 12-step trajectories, 2 x 64 LSTM, mirror loss on), same seed"""
    from learninghumanoidwalking_amd.envs import ENVIRONMENTS
    from learninghumanoidwalking_amd.ppo import PPO

    def run(on):
        monkeypatch.setenv("LHW_RNN_SEQ_FUSED", str(on))
        algo = PPO(ENVIRONMENTS["jvrc_walk"], _args(tmp_path, max_traj_len=12, num_procs=8, num_envs=8, minibatch_size=4, lstm_hidden=64), seed=11)
        for itr in range(2):
            algo.iterate(itr)
        assert algo.kernels.last_grad_fused == on
        return algo.kernels.theta.clone()
    a, b = run(0), run(1)
    assert torch.isfinite(a).all() and torch.equal(a, b)
