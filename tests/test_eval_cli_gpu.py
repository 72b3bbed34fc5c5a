"""`run_experiment.py train` logging the per-term episode statistics and the headless `run_experiment.py eval` on the GPU (the
reference's eval, /root/reference/run_experiment.py:245-292, without its viewer): reward_terms.csv, eval_summary.json, trajectory.npz."""
import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RX = os.path.join(ROOT, "run_experiment.py")


def _run(cmd, timeout):
    out = subprocess.run([sys.executable, RX] + cmd, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    return out


def _train(tmp_path, env, extra=()):
    logs = tmp_path / "logs"
    _run(["train", "--env", env, "--logdir", str(logs), "--n-itr", "2", "--num-envs", "16", "--max-traj-len", "20", "--minibatch-size", "64",
          "--eval-freq", "100", "--seed", "1", "--term-stats"] + list(extra), timeout=600)
    run = [d for d in os.listdir(logs) if d.endswith("_" + env)]
    assert len(run) == 1
    return logs, logs / run[0]


def _episode_returns(reward, done):
    """finished-episode returns of [T][K] float32 rewards segmented by done, summed in float64; and the sum of |r| over those steps"""
    rets, mags = [], []
    for k in range(reward.shape[1]):
        acc = mag = 0.0
        for t in range(reward.shape[0]):
            acc += float(reward[t, k])
            mag += abs(float(reward[t, k]))
            if done[t, k]:
                rets.append(acc)
                mags.append(mag)
                acc = mag = 0.0
    return np.array(rets), np.array(mags)


def test_train_logs_reward_terms_and_eval_replays_the_checkpoint(tmp_path):
    from learninghumanoidwalking_amd.batched_env import REWARD_TERMS, TASK_JVRC_WALK
    logs, run = _train(tmp_path, "jvrc_walk")
    with open(run / "reward_terms.csv") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["iteration", "episodes", "terminated", "truncated"] + list(REWARD_TERMS[TASK_JVRC_WALK])
    assert len(rows) == 3 and [r[0] for r in rows[1:]] == ["0", "1"]
    for r in rows[1:]:
        assert int(r[1]) == int(r[2]) + int(r[3]) > 0 and np.isfinite([float(x) for x in r[4:]]).all()

    out_dir, runs = tmp_path / "out", []
    for _ in range(2):                              # the same command twice
        res = _run(["eval", "--logdir", str(logs), "--num-envs", "8", "--ep-len", "1", "--seed", "3", "--out-dir", str(out_dir)], timeout=300)
        runs.append((res.stdout, (out_dir / "eval_summary.json").read_bytes()))
    assert runs[0] == runs[1]                       # counter-based RNG, no time stamps: byte-identical
    s = json.loads(runs[0][1])
    assert json.loads(runs[0][0][runs[0][0].index("{"):]) == s
    for key in ("checkpoint", "env", "seed", "episodes", "terminated", "truncated", "mean_return", "mean_length", "terms"):
        assert key in s, key
    assert s["env"] == "jvrc_walk" and s["seed"] == 3 and s["checkpoint"].endswith("actor_0.pt")      # (train saves where it evaluates: iteration 0)
    assert s["episodes"] >= 8 and s["episodes"] == s["terminated"] + s["truncated"]
    assert list(s["terms"]) == list(REWARD_TERMS[TASK_JVRC_WALK])
    T = s["control_steps"]
    assert T == 40                                  # 1 s of 0.025 s control steps
    tr = np.load(out_dir / "trajectory.npz")
    assert tr["qpos"].shape == (T, 8, 19) and tr["qvel"].shape == (T, 8, 18) and tr["action"].shape == (T, 8, 12)
    assert tr["reward"].shape == (T, 8) and tr["done"].shape == (T, 8) and np.isfinite(tr["qpos"]).all()
    assert (tr["done"] != 0).any(axis=0).all()      # every env finished an episode
    rets, mags = _episode_returns(tr["reward"], tr["done"])
    assert len(rets) == s["episodes"]
    err, bound = abs(rets.mean() - s["mean_return"]), 2.0 ** -23 * mags.sum() / len(rets)
    print("mean return: summary", s["mean_return"], "re-summed", rets.mean(), "err", err, "bound", bound)
    assert err <= bound
    np.testing.assert_allclose(sum(s["terms"].values()), s["mean_return"], rtol=1e-9)


def test_eval_of_a_recurrent_cartpole_checkpoint_writes_the_summary_only(tmp_path):
    logs, run = _train(tmp_path, "cartpole", extra=["--recurrent", "--minibatch-size", "8"])
    with open(run / "reward_terms.csv") as f:
        rows = list(csv.reader(f))
    assert rows[0][4:] == ["upright", "center", "velocity", "action"] and len(rows) == 3
    blobs = []
    for _ in range(2):
        out_dir = tmp_path / "out"
        _run(["eval", "--path", str(run), "--num-envs", "8", "--ep-len", "1", "--seed", "3", "--out-dir", str(out_dir)], timeout=300)
        blobs.append((out_dir / "eval_summary.json").read_bytes())
        assert not (out_dir / "trajectory.npz").exists()
    assert blobs[0] == blobs[1]
    s = json.loads(blobs[0])
    assert s["episodes"] >= 8 and s["control_steps"] == 50 and "not written" in s["trajectory"] and np.isfinite(s["mean_return"])
