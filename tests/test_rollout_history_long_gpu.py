"""The resident rollout of an env with a LONG observation history on the GPU: padded rows past 256 columns, which the in-wave policy step
takes through LDS 256 columns at a time (lhw_env_rollout_history, csrc/lhw_humanoid_rollout.hip: policy_step_wide), against the
launch-per-step pipeline itself -- PpoKernels.forward's per-layer GEMMs, BatchedEnv.step, batched_env.history_update.  Every stored value
equal, the weights after one update, the hand-over between the two paths, the job queue, the command line, and the plan a handle reports
for such a row.  Small batches: what the chunk loop can get wrong does not depend on the batch.  GPU twin of
tests/test_rollout_history_long.py (SIMT emulator); the helpers are tests/test_rollout_history_gpu.py's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.test_rollout_history_gpu import ROOT, _buffers, _history_yaml, _ppo

pytestmark = pytest.mark.gpu
NAMES = ("obs", "act", "logp", "tob_all", "rew", "done", "val", "vterm", "vfinal")


def _equal(a, b):
    for n, x, y in zip(NAMES, a, b):
        assert torch.equal(x, y), n


@pytest.mark.parametrize("env_name,width", [("jvrc_walk", 296), ("h1", 280)])
def test_long_history_rollout_is_the_launch_per_step_rollout_and_trains_to_the_same_weights(env_name, width, tmp_path, monkeypatch):
    """obs_history_len = 8 (two chunks), 5 envs, T = 6, episodes truncated at 4: LHW_ROLLOUT_MODE=resident against steps, same seed --
    every rollout buffer, the critic's values, the weights after one optimize() and the env state (h1: with it the observation-noise
    counter, which advances with every observation written)"""
    def run(mode):
        monkeypatch.setenv("LHW_ROLLOUT_MODE", mode)
        algo = _ppo(tmp_path, env_name, 8, 5, 6, seed=9, traj_len=4)
        assert algo.env.obs_dim == width
        algo.sample_parallel_with_workers()
        assert algo.rollout.last_mode == mode
        out = _buffers(algo.rollout)
        algo.optimize(0)
        torch.cuda.synchronize()
        theta, state = algo.kernels.theta.clone(), algo.env.get_state()
        # one more launch-per-step control step: the next observation (and its noise draw) is the same
        nxt = algo.env.step(torch.zeros(5, algo.env.act_dim, device="cuda"))[0].clone()
        return out, theta, state, nxt

    (a, wa, sa, na), (b, wb, sb, nb) = run("steps"), run("resident")
    _equal(a, b)
    assert torch.equal(wa, wb) and torch.equal(na, nb)
    np.testing.assert_array_equal(sa[0], sb[0])
    np.testing.assert_array_equal(sa[1], sb[1])
    done, obs, base = a[5], a[0], width // 8
    assert ((done & 2) != 0).any(), "no truncation / auto-reset inside the rollout"
    assert torch.equal((obs[1:, :, base:] == 0).all(dim=2), done != 0)      # an emptied history exactly behind an episode end


def test_long_history_rollout_through_the_job_queue(tmp_path, monkeypatch):
    """jvrc_step, obs_history_len = 7 (273 -> 276 columns), 5 envs on 2 assumed wave slots: a group's chunks of control steps run on
    whichever wave is free, against one wave per group"""
    monkeypatch.setenv("LHW_ROLLOUT_MODE", "resident")
    monkeypatch.setenv("LHW_ROLLOUT_SLOTS", "2")

    def run(chunk):
        monkeypatch.setenv("LHW_ROLLOUT_CHUNK", str(chunk))
        algo = _ppo(tmp_path, "jvrc_step", 7, 5, 6, seed=4, traj_len=4)
        algo.sample_parallel_with_workers()
        assert algo.rollout.last_mode == "resident" and algo.env.last_rollout_queued() == (chunk > 0)
        return _buffers(algo.rollout), algo.env.get_state(), algo.env.pop_fault_stats()

    (a, sa, fa), (b, sb, fb) = run(0), run(4)
    _equal(a, b)
    np.testing.assert_array_equal(sa[0], sb[0])
    np.testing.assert_array_equal(sa[1], sb[1])
    assert fa == fb == (0, 0) and (a[5] != 0).any()


@pytest.mark.parametrize("modes", [("resident", "steps"), ("steps", "resident")])
def test_the_two_paths_continue_each_other_at_a_long_history(modes, tmp_path, monkeypatch):
    """two consecutive collects on one env, one per path, against two launch-per-step collects on its twin, H = 8"""
    def run(ms):
        algo = _ppo(tmp_path, "jvrc_walk", 8, 5, 6, seed=11, traj_len=4)
        out = []
        for m in ms:
            monkeypatch.setenv("LHW_ROLLOUT_MODE", m)
            algo.sample_parallel_with_workers()
            assert algo.rollout.last_mode == m
            out.append(_buffers(algo.rollout))
        return out, algo.env.get_state()

    (a, sa), (b, sb) = run(("steps", "steps")), run(modes)
    for ra, rb in zip(a, b):
        _equal(ra, rb)
    np.testing.assert_array_equal(sa[0], sb[0])
    assert (a[1][5] != 0).any()


def test_training_from_the_command_line_takes_the_resident_path(tmp_path):
    """`run_experiment.py train` on an obs_history_len = 8 YAML in a child process, then `eval --out-dir` of the run: LHW_ROLLOUT_MODE=resident
    raises where the library declines, so exit status 0 says the long rows went through the resident kernel; and eval keeps the per-step
    record only on the resident path, which is where tests/test_rollout_history_gpu.py looks for the mode"""
    rx = os.path.join(ROOT, "run_experiment.py")

    def run(cmd):
        out = subprocess.run([sys.executable, rx] + cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, LHW_ROLLOUT_MODE="resident"))
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]

    logs, out_dir = tmp_path / "logs", tmp_path / "out"
    run(["train", "--env", "jvrc_walk", "--yaml", _history_yaml(tmp_path, 8), "--no-mirror", "--logdir", str(logs), "--n-itr", "1", "--num-envs", "16",
         "--max-traj-len", "20", "--minibatch-size", "64", "--eval-freq", "100", "--seed", "1"])
    run(["eval", "--logdir", str(logs), "--num-envs", "8", "--ep-len", "1", "--seed", "3", "--out-dir", str(out_dir)])
    s = json.loads((out_dir / "eval_summary.json").read_text())
    assert s["env"] == "jvrc_walk" and s["trajectory"] == "trajectory.npz", s["trajectory"]


@pytest.mark.parametrize("obs_dim,wide", [(259, False), (256, True)])
def test_plan_of_a_row_past_the_wide_strips(obs_dim, wide, monkeypatch):
    """A handle whose padded row is 260 columns wide reports per-layer GEMMs for the update and for inference with the wide strips switched
    on, and still makes the actor's [in][out] copy for the in-wave step; at 256 columns it reports the wide strips, as before"""
    from tests.test_update_plan_gpu import I_GEMM, I_STRIPS, INFER, U_GEMM, U_TRAIN, UPDATE, _call, _handle
    k = _handle(monkeypatch, obs_dim=obs_dim)
    _call(k, "wide", 1)
    plan = k.plan(k.max_rows)
    print(obs_dim, plan)
    assert {f: plan[f] for f in UPDATE} == (dict(U_TRAIN, wide=1) if wide else U_GEMM)
    assert {f: plan[f] for f in INFER} == (I_STRIPS if wide else dict(I_GEMM, actor_copies=1))
    k.begin_rollout()
    view = k.rollout_policy()
    k.end_rollout()
    assert view is not None and view.obs_pad == (obs_dim + 3) // 4 * 4
