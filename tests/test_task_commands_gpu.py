"""Task commands -- the settings of the fused tasks' command samplers and per-env pinned commands (lhw_env_set_task_commands /
lhw_env_get_task_commands / lhw_env_pin_commands / lhw_env_get_pinned_commands, include/lhw.h; `commands:` in an env's YAML;
`run_experiment.py eval --command`) -- on the GPU through the product BatchedEnv: the checks of tests/test_task_commands.py
(tests/task_commands_checks.py), the LSTM and history rollouts through the learner, and one `eval --command` run.  The reference has these
numbers as literals of tasks/walking_task.py:149-170,194-205 and stepping_task.py:261-334."""
import json
import os
import pickle
import subprocess
import sys
from functools import partial
from types import SimpleNamespace

import numpy as np
import pytest

from tests import task_commands_checks as C
from tests.task_shaping_checks import Backend, GpuRunner

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RX = os.path.join(ROOT, "run_experiment.py")

BACKEND = Backend(GpuRunner, device=0)


def test_fresh_env_reports_the_reference_values_and_no_pin():
    C.check_defaults(BACKEND)


@pytest.mark.parametrize("name", C.WALK_ENVS + ("jvrc_step",))
def test_setting_the_values_an_env_has_and_an_all_free_pin_change_no_bit(name):
    C.check_neutrality(BACKEND, name)


@pytest.mark.parametrize("name", C.WALK_ENVS)
def test_settings_against_the_oracle(name):
    C.check_settings_against_oracle(BACKEND, name)


def test_pinned_commands_against_the_oracle():
    C.check_pins_against_oracle(BACKEND)


@pytest.mark.parametrize("name", C.WALK_ENVS)
def test_resident_rollout_is_bitwise_the_launch_per_step_loop_under_commands(name):
    C.check_resident_equals_steps(BACKEND, name)


def test_resident_rollout_with_actuator_randomisation_is_bitwise_the_launch_per_step_loop_under_commands():
    C.check_resident_equals_steps(BACKEND, "jvrc_walk", act=True)


def _args(N, T, logdir, recurrent):
    return SimpleNamespace(gamma=0.99, lam=0.95, lr=3e-4, eps=1e-5, entropy_coeff=0.0, clip=0.2, minibatch_size=N if recurrent else N * T // 2,
                           epochs=1, max_traj_len=T, num_procs=N, num_envs=N, max_grad_norm=0.5, mirror_coeff=0.4, eval_freq=10**9,
                           recurrent=recurrent, imitate=None, learn_std=False, std_dev=0.4, no_mirror=True, continued=None, logdir=logdir,
                           device_index=0)


@pytest.mark.parametrize("kind", ["lstm", "history"])
def test_lstm_and_history_resident_rollouts_are_bitwise_the_launch_per_step_loop_under_commands(kind, tmp_path, monkeypatch):
    """jvrc_walk, 3 envs, T = 12 (the episode length: every rollout ends with an auto-reset), through the learner: a YAML with `commands:`
    (and obs_history_len = 3 for the history kind), env 0 pinned; a setter and two pin calls between two rollouts.  LHW_ROLLOUT_MODE =
    resident against steps, same seed: every rollout buffer and the env's state."""
    import torch
    from learninghumanoidwalking_amd.envs.jvrc_walk import JVRC_BASE_YAML, JvrcWalkSpec
    from learninghumanoidwalking_amd.ppo import PPO
    src = open(JVRC_BASE_YAML).read()
    assert "obs_history_len: 1" in src
    if kind == "history":
        src = src.replace("obs_history_len: 1", "obs_history_len: 3")
    s = C.SETTINGS
    src += ("\ncommands: {mode_probs: {standing: 0.25, inplace: 0.25, forward: 0.5}, switch_standing_every: 3, switch_walking_every: 3, "
            f"inplace_yaw_range: {list(s['inplace_yaw'])}, forward_speed_range: {list(s['forward_vx'])}, lateral_speed_range: {list(s['forward_vy'])}}}\n")
    (tmp_path / "commands.yaml").write_text(src)
    N, T = C.N, 12

    def run(mode):
        monkeypatch.setenv("LHW_ROLLOUT_MODE", mode)
        algo = PPO(partial(JvrcWalkSpec, yaml_path=str(tmp_path / "commands.yaml")), _args(N, T, str(tmp_path / "log"), kind == "lstm"), seed=9)
        env, ro = algo.env, algo.rollout
        assert env.get_task_commands() == dict(C.DEFAULTS, **dict(s, mode_cdf=(0.25, 0.5))) and env.history_len == (3 if kind == "history" else 1)
        env.pin_commands(*C.PIN0, envs=0)
        env.enable_task_inputs()
        out = []
        for n in range(2):
            algo.sample_parallel_with_workers()
            assert ro.last_mode == mode, ro.last_mode
            out.append([x.clone() for x in (ro.obs, ro.act, ro.logp, ro.rew, ro.done, ro.val)])
            if n == 0:
                env.set_task_commands(forward_vx=(0.6, 0.7), switch_walk_every=0)
                env.pin_commands(*C.PIN0_LATER, envs=0)
                env.pin_commands(*C.PIN0, envs=2)
        torch.cuda.synchronize()
        return out, env.get_state(), env.get_task_inputs()

    (a, sa, ra), (b, sb, rb) = run("steps"), run("resident")
    for x, y in zip(a, b):
        for n, u, v in zip(("obs", "act", "logp", "rew", "done", "val"), x, y):
            assert torch.equal(u, v), n
    np.testing.assert_array_equal(sa[0], sb[0])
    np.testing.assert_array_equal(sa[1], sb[1])
    for k in ra:
        np.testing.assert_array_equal(ra[k], rb[k], err_msg=k)
    assert list(rb["mode"][[0, 2]]) == [C.INPLACE, C.FORWARD] and rb["mode_ref"][0].tolist() == list(C.PIN0_LATER[1])
    assert (a[0][4] != 0).any(), "an auto-reset must be inside"
    # the pinned env's observation carries its command at every step of the first rollout, the reset at its end included
    cmd = a[0][0][:, 0, 31:37].cpu().numpy()
    np.testing.assert_array_equal(cmd, np.tile(np.float32([1, 0, 0, *C.PIN0[1]]), (T + 1, 1)))


def test_stair_height_schedule_moves_with_its_start():
    C.check_step_height_schedule(BACKEND)


def test_stepping_mode_thresholds_and_stair_height():
    C.check_step_modes_and_height(BACKEND)


def test_refused_calls_name_the_field_and_change_nothing():
    C.check_refusals(BACKEND)


# ---------------------------------------------------------------------------------------------------------------- eval --command
def _fresh_checkpoint(run, env_name):
    """a run directory as `train` leaves it, with freshly initialised weights: actor_0.pt / critic_0.pt and the pickled arguments"""
    sys.path.insert(0, ROOT)
    import run_experiment as rx
    from learninghumanoidwalking_amd.checkpoint import save_reference_checkpoint
    from learninghumanoidwalking_amd.envs import ENVIRONMENTS
    from learninghumanoidwalking_amd.ppo_kernels import reference_init
    import torch
    spec = ENVIRONMENTS[env_name]()
    run.mkdir(parents=True)
    args = rx.build_parser().parse_args(["--env", env_name, "--std-dev", "0.223"])
    with open(run / "experiment.pkl", "wb") as f:
        pickle.dump(args, f)
    tensors = reference_init(spec.obs_dim, spec.act_dim, 256, 0.223, generator_seed=0)
    save_reference_checkpoint(tensors, torch.as_tensor(spec.obs_mean, dtype=torch.float32), torch.as_tensor(spec.obs_std, dtype=torch.float32), False,
                              run / "actor_0.pt", run / "critic_0.pt")


def _eval(cmd, timeout=300):
    return subprocess.run([sys.executable, RX, "eval"] + cmd, capture_output=True, text=True, timeout=timeout)


def test_eval_command_pins_a_speed_per_env(tmp_path):
    """`eval --command forward:0.1..0.4`, 4 envs, one second, a freshly initialised checkpoint: per_env lists the four commands, every
    recorded mode_ref row is its env's command from the first step on, and the same command twice writes the same bytes"""
    from learninghumanoidwalking_amd import _lib
    import run_experiment as rx
    run, out_dir = tmp_path / "24-01-01-00-00-00-000_jvrc_walk", tmp_path / "out"
    _fresh_checkpoint(run, "jvrc_walk")
    blobs = []
    for _ in range(2):
        res = _eval(["--path", str(run), "--num-envs", "4", "--ep-len", "1", "--seed", "3", "--out-dir", str(out_dir), "--command", "forward:0.1..0.4"])
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
        with np.load(out_dir / "trajectory.npz") as z:
            blobs.append(((out_dir / "eval_summary.json").read_bytes(), {k: z[k].tobytes() for k in z.files}))
    assert blobs[0] == blobs[1]      # (the summary's bytes and every recorded array's; the .npz container itself carries time stamps)
    s = json.loads(blobs[0][0])
    assert s["command"] == "forward:0.1..0.4" and len(s["per_env"]) == 4 and s["control_steps"] == 40
    want = [0.1 + k * (0.4 - 0.1) / 3 for k in range(4)]
    assert [e["mode"] for e in s["per_env"]] == [2] * 4 and [e["mode_ref"] for e in s["per_env"]] == [[0.0, v, 0.0] for v in want]
    np.testing.assert_allclose(want, [0.1, 0.2, 0.3, 0.4], rtol=0, atol=1e-15)
    tr = np.load(out_dir / "trajectory.npz")
    T = s["control_steps"]
    m0, r0 = _lib.TASK_INPUT_FIELDS["mode"][0], _lib.TASK_INPUT_FIELDS["mode_ref"][0]
    rec = tr["task_inputs"]
    assert rec.shape[:2] == (T, 4)
    np.testing.assert_array_equal(rec[:, :, m0], 2.0)
    for k in range(4):
        np.testing.assert_array_equal(rec[:, k, r0:r0 + 3], np.tile([0.0, want[k], 0.0], (T, 1)))      # every step, the first included
    # return and length of every env's first episode, from the rollout's own rewards and flags, summed in float64 in time order
    for k, e in enumerate(s["per_env"]):
        ended = np.flatnonzero(tr["done"][:, k] != 0)
        L = int(ended[0]) + 1
        assert e["episode_length"] == L
        acc = 0.0
        for t in range(L):
            acc += float(tr["reward"][t, k])
        assert e["episode_return"] == acc
    # an env without a command to pin is refused by name
    for env_name in ("jvrc_step", "h1", "cartpole"):
        other = tmp_path / f"24-01-01-00-00-00-000_{env_name}"
        other.mkdir()
        for f in ("actor_0.pt", "critic_0.pt"):
            (other / f).write_bytes(b"")
        with open(other / "experiment.pkl", "wb") as f:
            pickle.dump(SimpleNamespace(env=env_name), f)
        with pytest.raises(SystemExit) as e:
            rx.run_eval(["--path", str(other), "--command", "standing"])
        assert "--command" in str(e.value) and env_name in str(e.value), e.value
