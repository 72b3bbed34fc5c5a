"""The wide instantiations of the MLP strip kernels (padded rows of 68 .. 256 columns: an observation history) on the chip.  GPU twin of
tests/test_emu_strip_wide.py, then the handle: PpoKernels(111, 12) (rows of 112 columns, jvrc_walk with a history of 3) with the switch
lhw_ppo_debug_set_strip_wide off -- one GEMM per layer, ppo_loss_kernel -- and on -- train strips, forward strips -- on ONE handle: equal
gradients, statistics and weights; the captured step; inference; one iteration of jvrc_walk end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.test_emu_mlp_strip import make_case
from tests.test_emu_strip_wide import TRAIN, policy_step_reference
from tests.test_emu_train_strip import check_equal, make_train_case, run_train_strip
from tests.test_optimizer_gpu import _ppo_batch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, A = 111, 12
_DT = {np.dtype(np.float32): torch.float32, np.dtype(np.int32): torch.int32}
_DEV = dict(ptr=lambda t: t.data_ptr(), alloc=lambda shape, t, fill: torch.full(shape, fill, dtype=_DT[np.dtype(t)], device="cuda"),
            dev=lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda())


@pytest.mark.parametrize("kw", TRAIN)
def test_wide_train_strip_equals_the_gemm_order(kw):
    from learninghumanoidwalking_amd import _lib
    L = _lib.lib()
    c = make_train_case(seed=3, **kw)
    un = run_train_strip(L, c, fused=0, **_DEV)
    fu = run_train_strip(L, c, fused=1, **_DEV)
    torch.cuda.synchronize()
    check_equal(c, un, fu, host=lambda t: t.cpu().numpy())


@pytest.mark.parametrize("Dp", [68, 128, 256])
@pytest.mark.parametrize("shape", ["small", "big"])
def test_wide_forward_strip_is_bit_identical_to_the_three_gemm_launches(Dp, shape, monkeypatch):
    """h1, h2 AND the read-out: at these widths the strip computes the GEMM path's single chain.  1000 rows: many slabs and a ragged one."""
    from learninghumanoidwalking_amd import _lib
    L = _lib.lib()
    monkeypatch.setenv("LHW_DEBUG_STRIP_SHAPE", shape)
    R, O, Op = 1000, 12, 16
    c = make_case(R=R, Dp=Dp, O=O, Op=Op, seed=Dp)
    d = {k: (torch.from_numpy(v).cuda() if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    p = lambda t: t.data_ptr()
    h1, h2, y = torch.full((R + 3, 256), 7.0, device="cuda"), torch.full((R + 3, 256), 7.0, device="cuda"), torch.full((R + 3, Op), 7.0, device="cuda")
    wt = torch.zeros((Dp + 256 + Op) * 256, device="cuda")
    _lib.check(L.lhw_debug_mlp_strip_forward(256, Dp, O, Op, p(d["w1"]), p(d["b1"]), p(d["w2"]), p(d["b2"]), p(d["w3"]), p(d["b3"]), p(d["x"]), Dp, R,
                                             p(h1), p(h2), p(y), p(wt), None))
    g1, g2, gy = torch.zeros(R, 256, device="cuda"), torch.zeros(R, 256, device="cuda"), torch.full((R, Op), 7.0, device="cuda")
    z = None
    _lib.check(L.lhw_debug_gemm(1, 1, 0, R, 256, Dp, p(d["x"]), Dp, p(d["w1"]), Dp, p(g1), 256, p(d["b1"]), 1, z, 0, 0, z, z, z, None))
    _lib.check(L.lhw_debug_gemm(1, 1, 0, R, 256, 256, p(g1), 256, p(d["w2"]), 256, p(g2), 256, p(d["b2"]), 1, z, 0, 0, z, z, z, None))
    _lib.check(L.lhw_debug_gemm(1, 1, 0, R, O, 256, p(g2), 256, p(d["w3"]), 256, p(gy), Op, p(d["b3"]), 0, z, 0, 0, z, z, z, None))
    torch.cuda.synchronize()
    assert (h1[R:] == 7.0).all() and (h2[R:] == 7.0).all() and (y[R:] == 7.0).all()
    assert torch.equal(h1[:R], g1) and torch.equal(h2[:R], g2)
    assert torch.equal(y[:R], gy), "the read-out is the GEMM's single chain over k"
    yref = policy_step_reference(L, c, **_DEV)
    torch.cuda.synchronize()
    assert torch.equal(y[:R, :O], yref[:, :O]), "and the plain policy launch's"


def _handle(learn_std, max_rows, mirror=False):
    from learninghumanoidwalking_amd.ppo_kernels import PpoKernels, reference_init
    kw = {}
    if mirror:      # a signed permutation of the 111 observation columns (and of the 12 actions)
        rs = np.random.default_rng(99)
        kw = dict(mirror_obs=(rs.permutation(D).astype(np.int32), rs.choice([-1.0, 1.0], size=D).astype(np.float32)),
                  mirror_act=(rs.permutation(A).astype(np.int32), rs.choice([-1.0, 1.0], size=A).astype(np.float32)))
    k = PpoKernels(D, A, hidden=256, max_rows=max_rows, learn_std=learn_std, entropy_coeff=0.01 if learn_std else 0.0, lr=1e-3, **kw)
    assert k.Dp == 112
    k.set_tensors(reference_init(D, A, 256, 0.223, generator_seed=7))
    return k


def _set(k, wide=None, fused=None):
    from learninghumanoidwalking_amd import _lib
    if wide is not None:
        _lib.check(k._L.lhw_ppo_debug_set_strip_wide(k._h, int(wide)))
    if fused is not None:
        _lib.check(k._L.lhw_ppo_debug_set_strip_fused(k._h, int(fused)))


@pytest.mark.parametrize("B,R,learn_std,mirror", [(256, 256, False, False), (256, 256, True, False), (33, 64, False, False), (33, 64, True, False),
                                                   (256, 256, True, True)])
def test_ppo_grad_and_apply_are_the_same_bits_with_the_wide_strips_on_and_off(B, R, learn_std, mirror):
    """(wide, fused) = (0, 1): the GEMM path; (1, 1): the train strips; (1, 0): the wide forward strip, ppo_loss_kernel, the backward strip."""
    k = _handle(learn_std, R, mirror)
    rs = np.random.default_rng(B + learn_std + 2 * mirror)
    k.set_obs_norm(rs.normal(size=D).astype(np.float32) * 0.1, (0.5 + rs.uniform(size=D)).astype(np.float32))
    xn, xm, act, logp, adv, ret, idx = _ppo_batch(k, rs, 512, 1, B)
    logp = logp + torch.tensor(rs.uniform(-0.5, 0.5, size=512).astype(np.float32)).cuda()      # ratios on both sides of the clip range
    theta0, res = k.theta.clone(), {}
    for wide, fused in ((0, 1), (1, 1), (1, 0)):
        _set(k, wide=wide, fused=fused)
        k.theta.copy_(theta0)
        for t in (k.grad, k.adam_m, k.adam_v, k.stats):
            t.zero_()
        k.adam_step = 0
        k.grad_minibatch(xn, xm if mirror else None, act, logp, adv, ret, idx[0])
        torch.cuda.synchronize()
        assert k.last_grad_fused == (wide and fused), "the path the switches ask for is the path that ran"
        grad, stats = k.grad.clone(), k.stats.clone()
        k.apply()
        torch.cuda.synchronize()
        res[wide, fused] = (grad, stats, k.theta.clone())
    ref = res[0, 1]
    assert ref[0].abs().sum() > 0 and 0 < float(ref[1][4]) < 1, "clip fraction strictly between 0 and 1"
    for key in ((1, 1), (1, 0)):
        assert torch.equal(ref[0], res[key][0]), ("flat gradient", key)
        assert torch.equal(ref[1], res[key][1]), ("loss statistics", key)
        assert torch.equal(ref[2], res[key][2]) and not torch.equal(ref[2], theta0), ("weights after lhw_ppo_apply", key)


def test_two_graph_steps_with_the_wide_strips_equal_the_two_call_gemm_path(monkeypatch):
    """lhw_ppo_step twice on a handle with the switch on == lhw_ppo_grad + lhw_ppo_apply twice on one with it off; then the switch toggled
    between two captured steps of ONE handle: the graph is recaptured and the second step runs the path asked for."""
    monkeypatch.delenv("LHW_PPO_GRAPH", raising=False)
    B = 256
    graph, eager = _handle(True, B), _handle(True, B)
    _set(graph, wide=1)
    _set(eager, wide=0)
    rs = np.random.default_rng(11)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        xn, xm, act, logp, adv, ret, idx = _ppo_batch(graph, rs, 1024, 4, B)
        for t in range(2):
            graph.step_minibatch(xn, None, act, logp, adv, ret, idx[t])
            eager.grad_minibatch(xn, None, act, logp, adv, ret, idx[t])
            eager.apply()
        stream.synchronize()
        assert graph.last_grad_fused == 1 and eager.last_grad_fused == 0
        for name in ("theta", "adam_m", "adam_v"):
            assert torch.equal(getattr(graph, name), getattr(eager, name)), name
        for t, wide in ((2, 0), (3, 1)):
            _set(graph, wide=wide)
            graph.step_minibatch(xn, None, act, logp, adv, ret, idx[t])
            eager.grad_minibatch(xn, None, act, logp, adv, ret, idx[t])
            eager.apply()
            stream.synchronize()
            assert graph.last_grad_fused == wide, "a toggled switch recaptures the step"
            for name in ("theta", "adam_m", "adam_v"):
                assert torch.equal(getattr(graph, name), getattr(eager, name)), (name, t)


def test_inference_is_the_same_bits_with_the_wide_strips_on_and_off():
    """PpoKernels.forward on 70 rows of 111 columns: per-layer GEMMs (off) == forward strips (on) == lhw_debug_policy_step's plain launch; and
    the one-launch policy step (no mu, no value)."""
    import ctypes
    from learninghumanoidwalking_amd._lib import LhwRolloutPolicy
    N = 70
    k = _handle(False, 128)
    rs = np.random.default_rng(4)
    k.set_obs_norm(rs.normal(size=D).astype(np.float32) * 0.3, (0.5 + rs.uniform(size=D)).astype(np.float32))
    obs = torch.from_numpy(rs.normal(size=(N, D)).astype(np.float32)).cuda()
    res = {}
    for wide in (0, 1):
        _set(k, wide=wide)
        mu, act, logp, value = k.forward(obs, seed=5, env_id_base=17, counter=9)
        _, act1, logp1, _ = k.forward(obs, seed=5, env_id_base=17, counter=9, want_value=False, want_mu=False)
        torch.cuda.synchronize()
        res[wide] = [t.clone() for t in (mu, value, act, logp, act1, logp1)]
    for a, b, name in zip(res[0], res[1], ("mu", "value", "act", "logp", "act (one launch)", "logp (one launch)")):
        assert torch.equal(a, b), name
    assert torch.equal(res[1][2], res[1][4]) and torch.equal(res[1][3], res[1][5])
    k.begin_rollout()
    view = k.rollout_policy(seed=5, counter=9)
    assert view is not None
    y, act, logp = torch.zeros(N, k.Op, device="cuda"), torch.zeros(N, A, device="cuda"), torch.zeros(N, device="cuda")
    assert k._L.lhw_debug_policy_step(ctypes.byref(view), obs.data_ptr(), N, 17, 9, y.data_ptr(), act.data_ptr(), logp.data_ptr(), None) == 0
    torch.cuda.synchronize()
    k.end_rollout()
    assert torch.equal(y[:, :A], res[1][0]) and torch.equal(act, res[1][2]) and torch.equal(logp, res[1][3])


_CHILD = r"""
import sys, torch
from functools import partial
from types import SimpleNamespace
sys.path.insert(0, sys.argv[1])
from learninghumanoidwalking_amd.envs import ENVIRONMENTS
from learninghumanoidwalking_amd.ppo import PPO
yaml_path, out, N, T = sys.argv[2], sys.argv[3], 64, 8
a = SimpleNamespace(gamma=0.99, lam=0.95, lr=3e-4, eps=1e-5, entropy_coeff=0.0, clip=0.2, minibatch_size=N * T // 2, epochs=1, max_traj_len=T,
                    num_procs=N, num_envs=N, max_grad_norm=0.5, mirror_coeff=0.4, eval_freq=10**9, recurrent=False, imitate=None,
                    learn_std=False, std_dev=0.4, no_mirror=True, continued=None, logdir=out + "_log", device_index=0)
algo = PPO(partial(ENVIRONMENTS["jvrc_walk"], yaml_path=yaml_path), a, seed=9)
assert algo.env.history_len == 3 and algo.kernels.Dp == 112
algo.sample_parallel_with_workers()
ro = algo.rollout
res = {n: getattr(ro, n).cpu().clone() for n in ("obs", "act", "logp", "tob_all", "rew", "done", "val", "vterm", "vfinal")}
algo.optimize(0)
torch.cuda.synchronize()
res["theta"] = algo.kernels.theta.cpu().clone()
res["fused"] = torch.tensor(algo.kernels.last_grad_fused)
res["wide"] = torch.tensor(int(algo.kernels.strip_wide))
res["mode"] = ro.last_mode
torch.save(res, out)
"""


def test_one_iteration_of_a_history_env_is_the_same_bits_with_the_wide_strips(tmp_path):
    """jvrc_walk with obs_history_len: 3, 64 envs, T = 8, --no-mirror: sample + optimize under LHW_STRIP_WIDE=1 and =0, each in a fresh child
    process (the switch is read when the handle is made)."""
    from learninghumanoidwalking_amd.envs.jvrc_walk import JVRC_BASE_YAML
    src = open(JVRC_BASE_YAML).read()
    assert "obs_history_len: 1" in src
    y = tmp_path / "jvrc_walk_h3.yaml"
    y.write_text(src.replace("obs_history_len: 1", "obs_history_len: 3"))
    script = tmp_path / "child.py"
    script.write_text(_CHILD)
    res = {}
    for sw in ("1", "0"):
        out = tmp_path / f"wide_{sw}.pt"
        r = subprocess.run([sys.executable, str(script), ROOT, str(y), str(out)], capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, LHW_STRIP_WIDE=sw, LHW_ROLLOUT_MODE="resident"))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        res[sw] = torch.load(out)
    assert int(res["1"]["wide"]) == 1 and int(res["0"]["wide"]) == 0
    assert int(res["1"]["fused"]) == 1 and int(res["0"]["fused"]) == 0
    assert res["1"]["mode"] == res["0"]["mode"] == "resident"
    for key in ("obs", "act", "logp", "tob_all", "rew", "done", "val", "vterm", "vfinal", "theta"):
        assert torch.equal(res["1"][key], res["0"][key]), key
