"""GPU twin of tests/test_policy_head.py: every call site of lhw_policy_sample on the device against the float64 restatement
(oracle/policy_head.py), pointwise, with the bounds of tests/policy_head_checks.py -- sample_kernel behind the per-layer GEMMs (float32
and fp16 operands) and behind lhw_rnn_forward, the fused read-out of the forward strip, the two reference policy launches, and the
rollouts PPO.sample_parallel_with_workers collects launch per step and resident (MLP, LSTM, observation histories of 3 and 8).

Every policy has zero read-out weights, so mu == b3 exactly whatever the observation and the operand type, and distinct per-action
stds set through set_tensors(...)["stds"].  Two cases: b3 = 0 with power-of-two stds (act == sd * z with no rounding besides z's), and
b3 random with non-dyadic stds.  Pointwise agreement carries the noise's statistics (tests/test_policy_head.py, part a).

Largest error / bound per path on an MI355X (action, log-density); no path needed more room than the derived bounds:
  forward: GEMMs + sample_kernel, fused strip read-out, strip + sample_kernel, fp16 GEMMs, fp16 strip, lhw_rnn_forward   0.996, 0.131
  forward with fp16 operands and no mu (7 and 64 rows)                                                                    0.935, 0.092
  lhw_debug_policy_step (37 and 296 columns), lhw_debug_lstm_policy_step                                                  0.996, 0.111
  PPO rollouts, steps and resident, MLP / LSTM / history 3 / history 8                                                    0.968, 0.077
(an action ratio just below 1 is a float32 rounding of z that all but reaches half an ulp, as on the host)"""
import ctypes
from functools import partial
from types import SimpleNamespace

import numpy as np
import pytest

from tests.policy_head_checks import CASES, COUNTER0, ENV_BASE, SEED, check_head, head_case, rollout_keys

pytestmark = pytest.mark.gpu
D, A = 37, 12


def _mlp_kernels(monkeypatch, obs_dim=D, max_rows=256, strip="2", infer_fp16=False, strip_fp16=False):
    import torch
    from learninghumanoidwalking_amd.ppo_kernels import PpoKernels, reference_init
    monkeypatch.setenv("LHW_MLP_STRIP", strip)      # (read once, when the handle is created)
    k = PpoKernels(obs_dim, A, hidden=256, max_rows=max_rows, learn_std=True)
    k.set_tensors(reference_init(obs_dim, A, 256, 0.223, generator_seed=3))
    rs = np.random.default_rng(0)
    k.set_obs_norm(rs.normal(size=obs_dim) * 0.3, 0.5 + rs.random(obs_dim))
    if strip_fp16:
        k.set_strip_fp16(True)
    if infer_fp16:
        k.set_inference_fp16(True)
    return k


def _set_head(k, case, names=("a_w3", "a_b3")):
    """zero read-out weights, the case's read-out bias and per-action stds"""
    import torch
    b3, sd, exact = head_case(case, A)
    k.set_tensors({names[0]: torch.zeros(A, 256), names[1]: torch.from_numpy(b3), "stds": torch.from_numpy(sd)})
    return b3, sd, exact


def _check_forward(k, rows, what, fused, **fwd):
    """PpoKernels.forward / RnnKernels.forward on `rows`-row batches at env_id_base 0 and 4096, sampled and deterministic, both cases; the
    130-row batch again as the sub-span [40, 73) at workspace row 65 (where the handle takes one)"""
    import torch
    g = torch.Generator().manual_seed(1)
    worst = np.zeros(2)
    for case in CASES:
        b3, sd, exact = _set_head(k, case, names=("a_wout", "a_bout") if k.recurrent else ("a_w3", "a_b3"))
        for R in rows:
            obs = (torch.randn(R, k.obs_dim, generator=g) * 1.5).cuda()
            for base, counter, det in ((0, 0, False), (ENV_BASE, COUNTER0, False), (ENV_BASE, COUNTER0 + 1, True)):
                spans = [(0, R, 0)] + ([(40, 73, 65)] if R == 130 and not k.recurrent else [])
                for a, b, ws in spans:
                    kw = dict(fwd, ws_row=ws) if not k.recurrent else dict(fwd)
                    mu, act, logp, _ = k.forward(obs[a:b], seed=SEED, env_id_base=base + a, counter=counter, deterministic=det, want_value=False, **kw)
                    torch.cuda.synchronize()
                    if mu is not None:
                        np.testing.assert_array_equal(mu.cpu().numpy(), np.broadcast_to(b3, (b - a, A)))      # mu == b3
                    env = np.arange(a, b, dtype=np.uint64) + np.uint64(base)
                    r = check_head(act.cpu().numpy(), logp.cpu().numpy(), b3, sd, SEED, env, counter, exact_fma=exact, deterministic=det,
                                   what=f"{what} {case} R={R} rows [{a}, {b}) base={base} det={det}")
                    worst = np.maximum(worst, r)
        assert k.recurrent or k.plan()["policy_step"] == int(fused), k.plan()
    print(f"{what}: error / bound: action {worst[0]:.3f}, log-density {worst[1]:.3f}")


def test_sample_kernel_behind_the_per_layer_gemms(monkeypatch):
    """PpoKernels.forward with LHW_MLP_STRIP=0: normalise, three GEMMs, sample_kernel (8 rows per block: 1, 7, 8, 9 and 130 rows)"""
    k = _mlp_kernels(monkeypatch, strip="0")
    assert k.plan()["infer_strips"] == 0
    _check_forward(k, (1, 7, 8, 9, 130), "forward, GEMMs + sample_kernel", fused=False)


def test_fused_read_out_of_the_forward_strip(monkeypatch):
    """PpoKernels.forward without mu and value: one strip launch, the Gaussian head on its read-out (64 rows per workgroup: 1, 63, 64, 65
    and 130 rows; the key is env_base + row0 + row)"""
    k = _mlp_kernels(monkeypatch)
    assert k.plan()["policy_step"] == 1
    _check_forward(k, (1, 63, 64, 65, 130), "forward, fused strip read-out", fused=True, want_mu=False)
    # with mu the same handle runs normalise, forward strip, sample_kernel
    _check_forward(k, (9, 130), "forward, strip + sample_kernel", fused=True)


@pytest.mark.parametrize("path", ["gemm", "strip"])
def test_fp16_inference(monkeypatch, path):
    """--infer-fp16 through the fp16 GEMMs and through the fp16 forward strip: with zero read-out weights mu stays b3, sample_kernel
    reads float32 means and stds"""
    k = _mlp_kernels(monkeypatch, strip="0" if path == "gemm" else "2", infer_fp16=True, strip_fp16=path == "strip")
    plan = k.plan()
    assert plan["infer_fp16_operands"] == 1 and plan["infer_strips"] == int(path == "strip") and plan["policy_step"] == 0
    _check_forward(k, (1, 8, 9, 65, 130), f"forward, fp16 {path}", fused=False)
    _check_forward(k, (7, 64), f"forward, fp16 {path}, no mu", fused=False, want_mu=False)


def test_sample_kernel_behind_the_lstm_forward():
    """RnnKernels.forward: the LSTM step, the read-out GEMM, sample_kernel"""
    import torch
    from learninghumanoidwalking_amd.rnn_kernels import RnnKernels, reference_init_lstm
    k = RnnKernels(D, A, hidden=256, seq_len=4, seq_cols=4, rollout_rows=130, learn_std=True)
    k.set_tensors(reference_init_lstm(D, A, 256, 0.2, generator_seed=2))
    _check_forward(k, (1, 7, 8, 9, 130), "lhw_rnn_forward + sample_kernel", fused=False)


def _check_debug_step(L, call, b3, sd, exact, R, det, what):
    import torch
    act, logp = torch.zeros(R, A, device="cuda"), torch.zeros(R, device="cuda")
    worst = np.zeros(2)
    for t in range(2):
        call(COUNTER0 + t, act, logp)
        torch.cuda.synchronize()
        r = check_head(act.cpu().numpy(), logp.cpu().numpy(), b3, sd, SEED, np.arange(R, dtype=np.uint64) + np.uint64(ENV_BASE), COUNTER0 + t,
                       exact_fma=exact, deterministic=det, what=f"{what} det={det}")
        worst = np.maximum(worst, r)
    return worst


@pytest.mark.parametrize("obs_dim", [D, 8 * D])      # the fused strip launch / mlp_policy_ref_kernel (rows wider than the strip's 64-column slab)
def test_reference_policy_launch(monkeypatch, obs_dim):
    """lhw_debug_policy_step on 65 rows from the actor view the resident rollout reads"""
    import torch
    from learninghumanoidwalking_amd import _lib
    L = _lib.lib()
    R = 65
    k = _mlp_kernels(monkeypatch, obs_dim=obs_dim, max_rows=128)
    obs = (torch.randn(R, obs_dim, generator=torch.Generator().manual_seed(2)) * 1.5).cuda()
    worst = np.zeros(2)
    for case in CASES:
        b3, sd, exact = _set_head(k, case)
        for det in (False, True):
            k.begin_rollout()
            view = k.rollout_policy(seed=SEED, counter=0, deterministic=det)
            assert view is not None
            y = torch.zeros(R, view.act_pad, device="cuda")

            def call(counter, act, logp):
                _lib.check(L.lhw_debug_policy_step(ctypes.byref(view), obs.data_ptr(), R, ENV_BASE, counter, y.data_ptr(), act.data_ptr(), logp.data_ptr(), None))
            worst = np.maximum(worst, _check_debug_step(L, call, b3, sd, exact, R, det, f"lhw_debug_policy_step D={obs_dim} {case}"))
            np.testing.assert_array_equal(y[:, :A].cpu().numpy(), np.broadcast_to(b3, (R, A)))
            k.end_rollout()
    print(f"lhw_debug_policy_step D={obs_dim}: error / bound: action {worst[0]:.3f}, log-density {worst[1]:.3f}")


def test_reference_lstm_policy_launch():
    """lhw_debug_lstm_policy_step on 65 rows"""
    import torch
    from learninghumanoidwalking_amd import _lib
    from learninghumanoidwalking_amd.rnn_kernels import RnnKernels, reference_init_lstm
    L = _lib.lib()
    R = 65
    k = RnnKernels(D, A, hidden=256, seq_len=4, seq_cols=4, rollout_rows=R, learn_std=True)
    k.set_tensors(reference_init_lstm(D, A, 256, 0.2, generator_seed=2))
    obs = (torch.randn(R, D, generator=torch.Generator().manual_seed(2)) * 1.5).cuda()
    reset = (torch.arange(R) % 3 == 0).to(torch.uint8).cuda()
    worst = np.zeros(2)
    for case in CASES:
        b3, sd, exact = _set_head(k, case, names=("a_wout", "a_bout"))
        for det in (False, True):
            view = k.rollout_policy(seed=SEED, counter=0, deterministic=det)
            assert view is not None
            y = torch.zeros(R, view.act_pad, device="cuda")

            def call(counter, act, logp):
                _lib.check(L.lhw_debug_lstm_policy_step(ctypes.byref(view), obs.data_ptr(), R, reset.data_ptr(), ENV_BASE, counter, y.data_ptr(), act.data_ptr(),
                                                        logp.data_ptr(), None))
            worst = np.maximum(worst, _check_debug_step(L, call, b3, sd, exact, R, det, f"lhw_debug_lstm_policy_step {case}"))
            np.testing.assert_array_equal(y[:, :A].cpu().numpy(), np.broadcast_to(b3, (R, A)))
    print(f"lhw_debug_lstm_policy_step: error / bound: action {worst[0]:.3f}, log-density {worst[1]:.3f}")


N_ENVS, T_STEPS, TRAJ = 5, 6, 4


def _ppo(tmp_path, kind):
    """PPO on jvrc_walk with 5 envs and rollouts of 6 control steps; its env re-made with episodes truncated at 4 (the noise key runs on
    through an auto-reset) and env_id_base 4096, its rollout with the 64-bit seed and a counter that starts at 1000"""
    from learninghumanoidwalking_amd.envs import ENVIRONMENTS
    from learninghumanoidwalking_amd.ppo import PPO, RecurrentRollout, Rollout
    H = dict(mlp=1, lstm=1, h3=3, h8=8)[kind]
    from learninghumanoidwalking_amd.envs.jvrc_walk import JVRC_BASE_YAML
    src = open(JVRC_BASE_YAML).read()
    assert "obs_history_len: 1" in src
    y = tmp_path / f"jvrc_walk_h{H}.yaml"
    y.write_text(src.replace("obs_history_len: 1", f"obs_history_len: {H}"))
    N, T = N_ENVS, T_STEPS
    args = SimpleNamespace(gamma=0.99, lam=0.95, lr=3e-4, eps=1e-5, entropy_coeff=0.0, clip=0.2, minibatch_size=N if kind == "lstm" else N * T // 2,
                           epochs=1, max_traj_len=T, num_procs=N, num_envs=N, max_grad_norm=0.5, mirror_coeff=0.4, eval_freq=10**9,
                           recurrent=kind == "lstm", imitate=None, learn_std=True, std_dev=0.223, no_mirror=True, continued=None,
                           logdir=str(tmp_path / "log"), device_index=0)
    algo = PPO(partial(ENVIRONMENTS["jvrc_walk"], yaml_path=str(y)), args, seed=9)
    assert algo.env.history_len == H and algo.env.obs_dim == H * D
    algo.env = algo.spec.make_batched(N, seed=algo.env_seed, device=algo.device, max_traj_len=TRAJ, env_id_base=ENV_BASE)
    assert algo.env.env_id_base == ENV_BASE
    if kind == "lstm":
        algo.rollout = RecurrentRollout(algo.env, algo.kernels, T, seed=SEED)
    else:
        algo.rollout = Rollout(algo.env, algo.kernels, T, seed=SEED, max_traj_len=T)
    algo.rollout.counter = COUNTER0
    return algo


@pytest.mark.parametrize("mode", ["steps", "resident"])
@pytest.mark.parametrize("kind", ["mlp", "lstm", "h3", "h8"])
def test_rollouts_of_the_learner(tmp_path, monkeypatch, kind, mode):
    """PPO.sample_parallel_with_workers, LHW_ROLLOUT_MODE = steps | resident, MLP / --recurrent / obs_history_len 3 and 8: two consecutive
    collects per case -- the second uses counters T .. 2T - 1 behind the first's -- with a truncation and an auto-reset inside"""
    monkeypatch.setenv("LHW_ROLLOUT_MODE", mode)
    algo = _ppo(tmp_path, kind)
    ro = algo.rollout
    worst = np.zeros(2)
    counter0 = COUNTER0
    for case in CASES:
        b3, sd, exact = _set_head(algo.kernels, case, names=("a_wout", "a_bout") if kind == "lstm" else ("a_w3", "a_b3"))
        for n in range(2):
            algo.sample_parallel_with_workers()
            assert ro.last_mode == mode and ro.counter == counter0 + T_STEPS
            env, counter = rollout_keys(T_STEPS, N_ENVS, ENV_BASE, counter0)
            act, logp, done = ro.act.cpu().numpy(), ro.logp.cpu().numpy(), ro.done.cpu().numpy()
            assert np.isfinite(ro.obs.cpu().numpy()).all()
            r = check_head(act, logp, b3, sd, SEED, env, counter, exact_fma=exact, what=f"{kind} {mode} {case} collect {n}")
            worst = np.maximum(worst, r)
            assert done[:-1].any(), "no episode end / auto-reset inside the rollout"
            counter0 += T_STEPS
    algo.sample_parallel_with_workers(deterministic=True)
    env, counter = rollout_keys(T_STEPS, N_ENVS, ENV_BASE, counter0)
    check_head(ro.act.cpu().numpy(), ro.logp.cpu().numpy(), b3, sd, SEED, env, counter, exact_fma=exact, deterministic=True, what=f"{kind} {mode} deterministic")
    print(f"PPO rollout {kind} {mode}: error / bound: action {worst[0]:.3f}, log-density {worst[1]:.3f}")
