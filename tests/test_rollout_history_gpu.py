"""The resident rollout of an env with an observation history on the GPU (lhw_env_rollout_history: obs_history_len > 1 of the
reference's YAML configs, envs/common/base_humanoid_env.py:53,177-197,274 -- the wavefront that advances an env shifts its history row
and evaluates the actor on the wide row itself) against the launch-per-step pipeline (per-layer GEMM forward, control-step launch,
batched_env.history_update): every stored value equal, the hand-over between the two, a reward-only task plug-in, the job queue and
the eval record.  GPU twin of tests/test_rollout_history.py (SIMT emulator)."""
import json
import os
import subprocess
import sys
from functools import partial
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(N, T, std=0.4, logdir="/tmp/lhw_test_history"):
    return SimpleNamespace(gamma=0.99, lam=0.95, lr=3e-4, eps=1e-5, entropy_coeff=0.0, clip=0.2, minibatch_size=N * T // 2, epochs=1,
                           max_traj_len=T, num_procs=N, num_envs=N, max_grad_norm=0.5, mirror_coeff=0.4, eval_freq=10**9,
                           recurrent=False, imitate=None, learn_std=False, std_dev=std, no_mirror=True, continued=None,
                           logdir=logdir, device_index=0)


def _history_yaml(tmp_path, H, env="jvrc_walk"):
    y = tmp_path / f"{env}_h{H}.yaml"
    if env == "h1_walk":      # (its file inherits h1_base.yaml from its own directory: written out whole)
        import yaml
        from learninghumanoidwalking_amd.envs.h1_walk import H1_WALK_YAML
        from learninghumanoidwalking_amd.envs.humanoid import load_config
        y.write_text(yaml.safe_dump(dict(load_config(H1_WALK_YAML), obs_history_len=H)))
        return str(y)
    if env in ("jvrc_walk", "jvrc_step"):
        from learninghumanoidwalking_amd.envs.jvrc_walk import JVRC_BASE_YAML as base
    else:
        from learninghumanoidwalking_amd.envs.h1 import H1_BASE_YAML as base
    src = open(base).read()
    assert "obs_history_len: 1" in src
    y.write_text(src.replace("obs_history_len: 1", f"obs_history_len: {H}"))
    return str(y)


def _ppo(tmp_path, env, H, N, T, seed, traj_len=None, task=None, std=0.4):
    """PPO on `env` with an obs_history_len = H YAML; traj_len: episodes shorter than the rollout (PPO itself ties the two together)"""
    from learninghumanoidwalking_amd.envs import ENVIRONMENTS
    from learninghumanoidwalking_amd.ppo import PPO, Rollout
    algo = PPO(partial(ENVIRONMENTS[env], yaml_path=_history_yaml(tmp_path, H, env)), _args(N, T, std=std, logdir=str(tmp_path / "log")), seed=seed, task=task)
    assert algo.env.history_len == H and algo.env.obs_dim == H * algo.env.base_obs_dim
    if traj_len is not None:
        assert task is None
        algo.env = algo.spec.make_batched(N, seed=algo.env_seed, device=algo.device, max_traj_len=traj_len, env_id_base=algo.env.env_id_base)
        if algo.term_stats_enabled:
            algo.env.enable_term_stats(True)
        algo.rollout = Rollout(algo.env, algo.kernels, T, seed=algo.rollout.seed, max_traj_len=T)
    return algo


def _buffers(ro):
    return [x.clone() for x in (ro.obs, ro.act, ro.logp, ro.tob_all, ro.rew, ro.done, ro.val, ro.vterm, ro.vfinal)]


def test_resident_history_rollout_is_the_launch_per_step_rollout_and_trains_to_the_same_weights(tmp_path, monkeypatch):
    """jvrc_walk, obs_history_len = 3 (rows of 111 -> 112 columns), 32 envs, T = 12, episodes truncated at 5: LHW_ROLLOUT_MODE=resident
    against steps, same seed -- every rollout buffer, the critic's values and the weights after one optimize()"""
    def run(mode):
        monkeypatch.setenv("LHW_ROLLOUT_MODE", mode)
        algo = _ppo(tmp_path, "jvrc_walk", 3, 32, 12, seed=9, traj_len=5)
        algo.sample_parallel_with_workers()
        assert algo.rollout.last_mode == mode
        out = _buffers(algo.rollout)
        algo.optimize(0)
        torch.cuda.synchronize()
        return out, algo.kernels.theta.clone(), algo.env.get_state()

    (a, wa, sa), (b, wb, sb) = run("steps"), run("resident")
    names = ("obs", "act", "logp", "tob_all", "rew", "done", "val", "vterm", "vfinal")
    for n, x, y in zip(names, a, b):
        assert torch.equal(x, y), n
    assert torch.equal(wa, wb)
    np.testing.assert_array_equal(sa[0], sb[0])
    done, obs = a[5], a[0]
    assert ((done & 2) != 0).any(), "no truncation / auto-reset inside the rollout"
    assert torch.equal((obs[1:, :, 37:] == 0).all(dim=2), done != 0)      # an emptied history exactly behind an episode end


@pytest.mark.parametrize("env_name", ["jvrc_step", "h1", "h1_walk"])
def test_resident_history_rollout_on_the_other_humanoid_envs(env_name, tmp_path, monkeypatch):
    """obs_history_len = 3 on the other three envs (padded rows of 120, 108 and 132 columns; h1 / h1_walk with observation noise and
    domain randomisation on, jvrc_step one env per wave), an odd batch, two rollouts with episodes ending inside"""
    def run(mode):
        monkeypatch.setenv("LHW_ROLLOUT_MODE", mode)
        algo = _ppo(tmp_path, env_name, 3, 33, 8, seed=7, traj_len=5)
        out = []
        for _ in range(2):
            algo.sample_parallel_with_workers()
            assert algo.rollout.last_mode == mode
            out.append(_buffers(algo.rollout))
        return out, algo.env.get_state(), algo.env.pop_fault_stats()

    (a, sa, fa), (b, sb, fb) = run("steps"), run("resident")
    for ra, rb in zip(a, b):
        for x, y in zip(ra, rb):
            assert torch.equal(x, y)
    np.testing.assert_array_equal(sa[0], sb[0])
    np.testing.assert_array_equal(sa[1], sb[1])
    assert fa == fb == (0, 0) and (a[0][5] != 0).any()


def test_in_wave_wide_policy_step_is_as_close_to_float64_as_the_gemm_forward(tmp_path, monkeypatch):
    """One deterministic policy step on 64 random rows of width 111: the in-wave means and PpoKernels.forward's means (per-layer GEMMs)
    are float32 evaluations of the same weights that can differ only in summation order, so against a float64 evaluation the in-wave
    error may be at most twice the launch-per-step error."""
    monkeypatch.setenv("LHW_ROLLOUT_MODE", "resident")
    N = 64
    algo = _ppo(tmp_path, "jvrc_walk", 3, N, 4, seed=3)
    k, env = algo.kernels, algo.env
    g = torch.Generator(device="cpu").manual_seed(5)
    mean, std = torch.as_tensor(algo.spec.obs_mean, dtype=torch.float32), torch.as_tensor(algo.spec.obs_std, dtype=torch.float32)
    rows = (mean + std * torch.randn(N, 111, generator=g)).cuda()
    ro = algo.rollout
    ro.obs[ro.T].copy_(env.reset())
    ro.started = True
    ro.obs[ro.T].copy_(rows)             # collect() continues from the last observation of the previous rollout
    ro.collect(deterministic=True)
    assert ro.last_mode == "resident" and torch.equal(ro.obs[0], rows)
    wave = ro.act[0].double().cpu()      # deterministic: the action is the mean
    mu, _, _, _ = k.forward(rows, deterministic=True, want_value=False)
    t = {n: v.double().cpu() for n, v in k.get_tensors().items()}
    x = ((rows.cpu() - mean) / std).double()      # (the float32 normalisation both evaluations share)
    h = torch.relu(x @ t["a_w1"][:, :111].T + t["a_b1"])
    h = torch.relu(h @ t["a_w2"].T + t["a_b2"])
    ref = h @ t["a_w3"][:12].T + t["a_b3"][:12]
    e_wave, e_gemm = (wave - ref).abs().max().item(), (mu.double().cpu() - ref).abs().max().item()
    print(f"worst |mean - float64|: in-wave {e_wave:.3e}, launch-per-step GEMMs {e_gemm:.3e}; equal: {torch.equal(ro.act[0], mu)}")
    assert e_wave <= 2 * e_gemm


def test_launch_per_step_rollouts_continue_a_resident_history_rollout(tmp_path, monkeypatch):
    """T resident steps, then T launch-per-step steps on one env, against 2 T launch-per-step steps on its twin: BatchedEnv.rollout leaves
    the env's own copy of the full observation equal to obs[T]"""
    def run(modes):
        algo = _ppo(tmp_path, "jvrc_walk", 3, 32, 6, seed=11, traj_len=4)
        out = []
        for m in modes:
            monkeypatch.setenv("LHW_ROLLOUT_MODE", m)
            algo.sample_parallel_with_workers()
            assert algo.rollout.last_mode == m
            out.append(_buffers(algo.rollout))
        return out, algo.env.get_state()

    (a, sa), (b, sb) = run(["steps", "steps", "steps"]), run(["resident", "steps", "resident"])
    for ra, rb in zip(a, b):
        for x, y in zip(ra, rb):
            assert torch.equal(x, y)
    np.testing.assert_array_equal(sa[0], sb[0])
    assert (a[1][5] != 0).any()


def test_reward_only_task_plug_in_on_a_history_env_keeps_the_resident_rollout(tmp_path, monkeypatch):
    """VectorWalkingTask never touches an observation: it constructs on the H = 3 env, the rollout runs resident with the record of every
    control step, and its rewards are the fused reward's (the tolerance of tests/test_task_hook_gpu.py for this task)"""
    from learninghumanoidwalking_amd.task_hook import VectorWalkingTask
    monkeypatch.setenv("LHW_ROLLOUT_MODE", "resident")
    fused = _ppo(tmp_path, "jvrc_walk", 3, 24, 10, seed=5, std=0.3)
    vect = _ppo(tmp_path, "jvrc_walk", 3, 24, 10, seed=5, std=0.3, task=lambda spec, dev: VectorWalkingTask(spec, dev))
    assert vect.rollout.reward_only
    for algo in (fused, vect):
        algo.sample_parallel_with_workers()
        assert algo.rollout.last_mode == "resident"
    assert torch.equal(fused.rollout.obs, vect.rollout.obs) and torch.equal(fused.rollout.done, vect.rollout.done)
    np.testing.assert_allclose(vect.rollout.rew.cpu().numpy(), fused.rollout.rew.cpu().numpy(), rtol=0, atol=1e-6)
    # a task that decides terminations itself resets through the env, which knows nothing of the history: still refused
    with pytest.raises(NotImplementedError, match="decides terminations"):
        _ppo(tmp_path, "jvrc_walk", 3, 24, 10, seed=5, task=lambda spec, dev: VectorWalkingTask(spec, dev, height_limits=(0.6, 1.4000001)))


def test_history_rollout_through_the_job_queue_is_bitwise_the_one_wave_per_group_rollout(tmp_path, monkeypatch):
    """jvrc_step, obs_history_len = 2, 64 envs on 48 assumed wave slots: a group's chunks run on whichever wave is free, the shifted rows
    travel to the next chunk's wave under the fences that carry obs[t + 1] without a history"""
    monkeypatch.setenv("LHW_ROLLOUT_MODE", "resident")
    monkeypatch.setenv("LHW_ROLLOUT_SLOTS", "48")

    def run(chunk):
        monkeypatch.setenv("LHW_ROLLOUT_CHUNK", str(chunk))
        algo = _ppo(tmp_path, "jvrc_step", 2, 64, 14, seed=4, traj_len=6)
        out = []
        for _ in range(2):
            algo.sample_parallel_with_workers()
            assert algo.rollout.last_mode == "resident" and algo.env.last_rollout_queued() == (chunk > 0)
            out.append(_buffers(algo.rollout))
        return out, algo.env.get_state(), algo.env.pop_fault_stats()

    (a, sa, fa), (b, sb, fb) = run(0), run(3)
    for ra, rb in zip(a, b):
        for x, y in zip(ra, rb):
            assert torch.equal(x, y)
    np.testing.assert_array_equal(sa[0], sb[0])
    np.testing.assert_array_equal(sa[1], sb[1])
    assert fa == fb == (0, 0) and (a[0][5] != 0).any()


def test_eval_of_a_history_run_writes_the_trajectory(tmp_path):
    """`run_experiment.py eval --out-dir` keeps the per-step record only on the resident path: an obs_history_len = 2 run now has one"""
    rx = os.path.join(ROOT, "run_experiment.py")

    def run(cmd):
        out = subprocess.run([sys.executable, rx] + cmd, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]

    logs, out_dir = tmp_path / "logs", tmp_path / "out"
    run(["train", "--env", "jvrc_walk", "--yaml", _history_yaml(tmp_path, 2), "--no-mirror", "--logdir", str(logs), "--n-itr", "1", "--num-envs", "16",
         "--max-traj-len", "20", "--minibatch-size", "64", "--eval-freq", "100", "--seed", "1"])
    run(["eval", "--logdir", str(logs), "--num-envs", "8", "--ep-len", "1", "--seed", "3", "--out-dir", str(out_dir)])
    s = json.loads((out_dir / "eval_summary.json").read_text())
    assert s["env"] == "jvrc_walk" and s["trajectory"] == "trajectory.npz", s["trajectory"]
    tr = np.load(out_dir / "trajectory.npz")
    T = s["control_steps"]
    assert tr["qpos"].shape == (T, 8, 19) and tr["action"].shape == (T, 8, 12) and np.isfinite(tr["qpos"]).all()
