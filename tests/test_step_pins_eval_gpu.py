"""`run_experiment.py eval --footsteps` on the GPU: every env of a jvrc_step run pinned to FORWARD with a stair height of its own, the
summary's per-env report, the recorded terrain, and a run without the flag that reports none of it."""
import json
import os
import pickle
import sys
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_eval_footsteps_pins_a_stair_height_per_env(tmp_path):
    from tests.test_eval_cli_gpu import _run, _train
    _, run = _train(tmp_path, "jvrc_step")
    out_dir = tmp_path / "out"
    base = ["eval", "--path", str(run), "--num-envs", "4", "--ep-len", "0.15", "--seed", "3", "--out-dir", str(out_dir)]
    _run(base + ["--footsteps", "forward:0.0..0.08"], timeout=300)
    s = json.loads((out_dir / "eval_summary.json").read_text())
    want = [0.0 + k * (0.08 - 0.0) / 3 for k in range(4)]
    T = s["control_steps"]
    assert T == 6 and s["footsteps"] == "forward:0.0..0.08" and len(s["per_env"]) == 4
    assert [e["height"] for e in s["per_env"]] == want and [e["mode"] for e in s["per_env"]] == ["forward"] * 4
    assert [e["nseq"] for e in s["per_env"]] == [0] * 4
    assert isinstance(s["contact_overflow"], int) and isinstance(s["diverged"], int)
    tr = np.load(out_dir / "trajectory.npz")
    assert tr["terrain_seq"].shape == (T, 4, 20, 4) and (tr["terrain_nseq"] == 20).all() and (tr["terrain_floor_z"] == -2.0).all()
    for k, e in enumerate(s["per_env"]):
        ended = np.flatnonzero(tr["done"][:, k] != 0)
        L = int(ended[0]) + 1 if ended.size else T
        assert e["length"] == L
        acc = 0.0
        for t in range(L):
            acc += float(tr["reward"][t, k])
        assert e["return"] == acc
        assert e["targets_reached"] == int(tr["step_task_inputs"][:L, k, 16].max())
        for t in range(L):      # the terrain in force during the first episode: every step rises by the env's height or not at all
            dz = np.diff(tr["terrain_seq"][t, k, :, 2])
            np.testing.assert_allclose(dz[dz != 0], want[k], rtol=0, atol=1e-12)      # (z is a running sum of the height: a rounding per step)
            assert np.count_nonzero(dz) >= (15 if want[k] else 0)      # (19 steps, the first two to three of them flat)
    # without the flag: the parent's summary, none of the new keys
    _run(base, timeout=300)
    plain = json.loads((out_dir / "eval_summary.json").read_text())
    assert not {"footsteps", "per_env", "contact_overflow", "diverged"} & set(plain)
    assert set(plain) == set(s) - {"footsteps", "per_env", "contact_overflow", "diverged"}
    # an env whose command is no footstep plan is refused by name
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import run_experiment as rx
    for env_name in ("jvrc_walk", "h1", "cartpole"):
        other = tmp_path / f"24-01-01-00-00-00-000_{env_name}"
        other.mkdir()
        for f in ("actor_0.pt", "critic_0.pt"):
            (other / f).write_bytes(b"")
        with open(other / "experiment.pkl", "wb") as f:
            pickle.dump(SimpleNamespace(env=env_name), f)
        with pytest.raises(SystemExit) as e:
            rx.run_eval(["--path", str(other), "--footsteps", "forward"])
        assert "--footsteps" in str(e.value) and env_name in str(e.value), e.value
