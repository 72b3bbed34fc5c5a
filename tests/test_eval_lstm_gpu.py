"""`run_experiment.py eval --out-dir` of a humanoid LSTM checkpoint: the resident LSTM rollout (lhw_env_rollout_lstm) exports the
per-step record, so trajectory.npz is written as for feed-forward actors (the reference's eval of a --recurrent run,
/root/reference/run_experiment.py:179, 245-292, without its viewer)."""
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


def test_eval_of_a_recurrent_jvrc_walk_checkpoint_writes_the_trajectory(tmp_path):
    logs = tmp_path / "logs"
    _run(["train", "--env", "jvrc_walk", "--recurrent", "--logdir", str(logs), "--n-itr", "2", "--num-envs", "16", "--max-traj-len", "20",
          "--minibatch-size", "8", "--eval-freq", "100", "--seed", "1"], timeout=900)
    out_dir, blobs = tmp_path / "out", []
    for _ in range(2):                              # the same command twice
        _run(["eval", "--logdir", str(logs), "--num-envs", "8", "--ep-len", "1", "--seed", "3", "--out-dir", str(out_dir)], timeout=600)
        blobs.append((out_dir / "eval_summary.json").read_bytes())
    assert blobs[0] == blobs[1]
    s = json.loads(blobs[0])
    assert s["env"] == "jvrc_walk" and s["trajectory"] == "trajectory.npz"
    assert s["episodes"] >= 8 and s["episodes"] == s["terminated"] + s["truncated"] and np.isfinite(s["mean_return"])
    T = s["control_steps"]
    assert T == 40                                  # 1 s of 0.025 s control steps
    tr = np.load(out_dir / "trajectory.npz")
    assert tr["qpos"].shape == (T, 8, 19) and tr["qvel"].shape == (T, 8, 18) and tr["action"].shape == (T, 8, 12)
    assert tr["reward"].shape == (T, 8) and tr["done"].shape == (T, 8) and float(tr["control_dt"]) == 0.025
    assert np.isfinite(tr["qpos"]).all() and np.isfinite(tr["action"]).all()
    assert (tr["done"] != 0).any(axis=0).all()      # every env finished an episode
