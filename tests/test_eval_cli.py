"""`run_experiment.py eval` without a GPU: checkpoint resolution as the reference's eval does it (/root/reference/run_experiment.py:245-269:
an actor file, a run directory -> latest actor, --logdir -> latest run -> latest actor; critic and experiment.pkl beside it) on a
fabricated directory tree, and the exit without a device."""
import os
import pickle
import subprocess
import sys
from types import SimpleNamespace

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tree(tmp_path):
    old, new = tmp_path / "24-01-01-00-00-00-000_jvrc_walk", tmp_path / "24-06-01-00-00-00-000_jvrc_walk"
    for run, itrs in ((old, (0, 99)), (new, (0, 9, 19))):
        run.mkdir()
        for i in itrs:
            (run / f"actor_{i}.pt").write_bytes(b"")
            (run / f"critic_{i}.pt").write_bytes(b"")
        (run / "actor.pt").write_bytes(b"")
        (run / "critic.pt").write_bytes(b"")
        with open(run / "experiment.pkl", "wb") as f:
            pickle.dump(SimpleNamespace(env="jvrc_walk"), f)
    (tmp_path / "notes").mkdir()          # a directory that is not a run
    return old, new


def test_eval_resolves_checkpoints_like_the_reference(tmp_path):
    sys.path.insert(0, ROOT)
    import run_experiment as rx
    old, new = _tree(tmp_path)
    assert rx.resolve_checkpoint(None, tmp_path) == (new / "actor_19.pt", new / "critic_19.pt", new / "experiment.pkl")   # 19 > 9: by number
    assert rx.resolve_checkpoint(old, None) == (old / "actor_99.pt", old / "critic_99.pt", old / "experiment.pkl")
    assert rx.resolve_checkpoint(old / "actor.pt", None) == (old / "actor.pt", old / "critic.pt", old / "experiment.pkl")
    assert rx.resolve_checkpoint(new / "actor_9.pt", None)[1] == new / "critic_9.pt"
    os.remove(new / "experiment.pkl")
    assert rx.resolve_checkpoint(None, tmp_path)[0] == old / "actor_99.pt"       # a directory without the pickle is not a run
    with pytest.raises(SystemExit, match="experiment.pkl is missing"):
        rx.resolve_checkpoint(new, None)
    os.remove(old / "critic_99.pt")
    with pytest.raises(SystemExit, match="critic_99.pt is missing"):
        rx.resolve_checkpoint(old, None)
    for bad in ((None, None), (old, tmp_path)):
        with pytest.raises(SystemExit, match="exactly one"):
            rx.resolve_checkpoint(*bad)
    with pytest.raises(SystemExit, match="no run directory"):
        rx.resolve_checkpoint(None, tmp_path / "notes")
    with pytest.raises(SystemExit, match="neither"):
        rx.resolve_checkpoint(new / "critic_9.pt", None)


def test_eval_without_a_gpu_exits_with_the_mi355x_message(tmp_path):
    _tree(tmp_path)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="")      # hide any device
    out = subprocess.run([sys.executable, os.path.join(ROOT, "run_experiment.py"), "eval", "--logdir", str(tmp_path)],
                         capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode != 0
    assert "MI355X only" in out.stderr and "Traceback" not in out.stderr, out.stderr[-2000:]
