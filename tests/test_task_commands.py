"""Task commands -- the settings of the fused tasks' command samplers and per-env pinned commands (lhw_env_set_task_commands /
lhw_env_get_task_commands / lhw_env_pin_commands / lhw_env_get_pinned_commands, include/lhw.h; `commands:` in an env's YAML;
`run_experiment.py eval --command`) -- on the SIMT emulator, plus the host-only parts (YAML -> spec -> make_batched, the command spec of
eval).  The reference has these numbers as literals of tasks/walking_task.py:149-170,194-205 and
stepping_task.py:261-334; what other values must give is stated by the oracle with those methods overridden
(tests/task_commands_checks.py).  CPU twin of tests/test_task_commands_gpu.py."""
import os
import sys

import numpy as np
import pytest

import torch

from tests import emu
from tests import task_commands_checks as C
from tests.task_shaping_checks import Backend, EmuRunner

BACKEND = Backend(EmuRunner, device=torch.device("cpu"), library=emu.lib)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def _commanded(env):
    """non-default settings plus a partial pin"""
    env.set_task_commands(**C.SETTINGS)
    env.pin_commands(*C.PIN0, envs=0)


def _between(env):
    """the setter and two pin calls between two rollouts"""
    env.set_task_commands(forward_vx=(0.6, 0.7), switch_walk_every=0)
    env.pin_commands(*C.PIN0_LATER, envs=0)
    env.pin_commands(*C.PIN0, envs=2)


def test_lstm_resident_rollout_is_bitwise_the_launch_per_step_loop_under_commands():
    from tests import test_rollout_lstm as RL
    from tests.test_rollout_resident import _same
    spec, T = C.spec_of("jvrc_walk"), 6
    envs, pols = RL._pair(spec, C.N, 11, 5, max_traj_len=5)
    for e in envs:
        _commanded(e)
    obs0 = [e.reset().copy() for e in envs]
    reset0 = np.ones(C.N, np.uint8)
    a = RL._per_step(envs[0], pols[0], T, obs0[0], reset0)
    b = RL._resident(envs[1], pols[1], T, obs0[1], reset0)
    _same(a, b)
    np.testing.assert_array_equal(a["obs"][:, 0, 31:37], np.tile(np.float32([1, 0, 0, *C.PIN0[1]]), (T + 1, 1)))      # env 0 follows its pin
    assert (a["done"] != 0).any(), "an auto-reset must be inside"
    for e, p in zip(envs, pols):
        _between(e)
        p.view.counter += T
    r0 = (a["done"][T - 1] != 0).astype(np.uint8)
    a2 = RL._per_step(envs[0], pols[0], T, a["obs"][T], r0)
    b2 = RL._resident(envs[1], pols[1], T, b["obs"][T], r0)
    _same(a2, b2)
    np.testing.assert_array_equal(a2["obs"][1:, 0, 31:37], np.tile(np.float32([0, 1, 0, *C.PIN0_LATER[1]]), (T, 1)))
    for x, y in zip(envs[0].get_state(), envs[1].get_state()):
        np.testing.assert_array_equal(x, y)
    RL._same_state(pols[0], pols[1])


def test_history_resident_rollout_is_bitwise_the_launch_per_step_loop_under_commands():
    from tests import test_rollout_history as RH
    from tests.test_rollout_resident import NumpyActor
    spec, T, H = C.spec_of("jvrc_walk"), 6, 3
    envs = RH._pair(spec, H, C.N, seed=11, max_traj_len=5)
    for e in envs:
        _commanded(e)
    pol = NumpyActor(H * 37, 12, seed=5, scale=2.0)
    obs0 = RH._first_obs(envs, H)
    a = RH._reference(envs[0], pol, T, obs0[0], H)
    b = RH._resident(envs[1], pol, T, obs0[1], H)
    RH._same(a, b)
    np.testing.assert_array_equal(b["obs"][:, 0, 31:37], np.tile(np.float32([1, 0, 0, *C.PIN0[1]]), (T + 1, 1)))
    assert (a["done"] != 0).any(), "an auto-reset must be inside"
    for e in envs:
        _between(e)
    pol.view.counter += T
    a2 = RH._reference(envs[0], pol, T, a["obs"][T], H)
    b2 = RH._resident(envs[1], pol, T, b["obs"][T], H)
    RH._same(a2, b2)
    np.testing.assert_array_equal(b2["obs"][1:, 0, 31:37], np.tile(np.float32([0, 1, 0, *C.PIN0_LATER[1]]), (T, 1)))
    RH._same_state(*envs)


def test_stair_height_schedule_moves_with_its_start():
    C.check_step_height_schedule(BACKEND)


def test_stepping_mode_thresholds_and_stair_height():
    C.check_step_modes_and_height(BACKEND)


def test_refused_calls_name_the_field_and_change_nothing():
    C.check_refusals(BACKEND)


# ---------------------------------------------------------------------------------------------------------------- spec / YAML (no library)
def _yaml(tmp_path, name, text):
    from learninghumanoidwalking_amd.envs import ENVIRONMENTS
    base = ENVIRONMENTS[name]().yaml_path
    path = tmp_path / f"{name}_commands.yaml"
    path.write_text(f"inherits: {base}\n" + text)      # (load_config: the child's keys win; an absolute parent path is taken as it is)
    return ENVIRONMENTS[name](yaml_path=str(path))


def test_yaml_keys_map_to_the_struct(tmp_path):
    from learninghumanoidwalking_amd import _lib
    spec = _yaml(tmp_path, "jvrc_walk", "commands: {mode_probs: {standing: 0.25, inplace: 0.25, forward: 0.5}, inplace_yaw_range: [-0.2, 0.9], "
                                        "forward_speed_range: [0.3, 0.8], lateral_speed_range: [-0.1, 0.25], switch_standing_every: 50, switch_walking_every: 0}\n")
    assert spec.commands() == dict(mode_cdf=(0.25, 0.5), inplace_yaw=(-0.2, 0.9), forward_vx=(0.3, 0.8), forward_vy=(-0.1, 0.25),
                                   switch_stand_every=50, switch_walk_every=0)
    assert "commands" not in spec.env_args()[2]      # (a setting of the env, not of its creation)
    # the struct the setter builds from it holds the values in the stated order
    c = _lib.task_commands_struct(dict(_lib.DEFAULT_TASK_COMMANDS, **spec.commands()))
    assert _lib.task_commands_dict(c) == dict(_lib.DEFAULT_TASK_COMMANDS, **spec.commands())
    assert [n for n, _ in c._fields_] == ["mode_cdf", "inplace_yaw", "forward_vx", "forward_vy", "switch_stand_every", "switch_walk_every",
                                          "step_mode_cdf", "step_height_start", "step_height_span", "step_height_max"]
    # the reference's probabilities, summed here, give the thresholds an env starts with (a sum need not hit a literal -- 0.1 + 0.2 != 0.3 --
    # which is why the ABI takes thresholds; these do)
    assert _lib.cdf_from_probs(dict(standing=0.6, inplace=0.2, forward=0.2), _lib.COMMAND_MODES) == _lib.DEFAULT_TASK_COMMANDS["mode_cdf"]
    assert _lib.cdf_from_probs(dict(curved=0.15, standing=0.05, backward=0.2, lateral=0.3, forward=0.3), _lib.STEP_COMMAND_MODES) == \
        _lib.DEFAULT_TASK_COMMANDS["step_mode_cdf"]
    # one key alone: only that setting is handed on
    assert _yaml(tmp_path, "h1_walk", "commands: {forward_speed_range: [0.8, 0.8]}\n").commands() == dict(forward_vx=(0.8, 0.8))
    spec = _yaml(tmp_path, "jvrc_step", "commands: {mode_probs: {curved: 0.1, standing: 0.1, backward: 0.1, lateral: 0.2, forward: 0.5}, "
                                        "stair_height: {start_iteration: 0, span_iterations: 100, max: 0.05}}\n")
    got = spec.commands()
    np.testing.assert_allclose(got.pop("step_mode_cdf"), (0.1, 0.2, 0.3, 0.5), rtol=0, atol=1e-15)
    assert got == dict(step_height_start=0.0, step_height_span=100.0, step_height_max=0.05)


@pytest.mark.parametrize("name,text,error", [
    ("jvrc_walk", "commands: {mode_prob: {standing: 1, inplace: 0, forward: 0}}", KeyError),
    ("jvrc_walk", "commands: {mode_probs: {standing: 0.5, forward: 0.5}}", KeyError),
    ("jvrc_walk", "commands: {mode_probs: {standing: 0.5, inplace: 0.2, forward: 0.2}}", ValueError),
    ("jvrc_walk", "commands: {mode_probs: {standing: 1.5, inplace: -0.5, forward: 0.0}}", ValueError),
    ("jvrc_walk", "commands: {forward_speed_range: [0.8, 0.3]}", ValueError),
    ("jvrc_walk", "commands: {lateral_speed_range: 0.3}", ValueError),
    ("jvrc_walk", "commands: {inplace_yaw_range: [0.1, .nan]}", ValueError),
    ("h1_walk", "commands: {switch_standing_every: -1}", ValueError),
    ("h1_walk", "commands: {switch_walking_every: 2.5}", ValueError),
    ("jvrc_walk", "commands: {stair_height: {max: 0.2}}", KeyError),
    ("jvrc_step", "commands: {forward_speed_range: [0.1, 0.2]}", KeyError),
    ("jvrc_step", "commands: {stair_height: {span: 100}}", KeyError),
    ("jvrc_step", "commands: {stair_height: {span_iterations: 0}}", ValueError),
    ("jvrc_step", "commands: {mode_probs: {standing: 0.5, inplace: 0.25, forward: 0.25}}", KeyError),
    ("h1", "commands: {mode_probs: {standing: 1, inplace: 0, forward: 0}}", ValueError),
])
def test_yaml_mistakes_are_refused_with_the_file_named(tmp_path, name, text, error):
    with pytest.raises(error) as e:
        _yaml(tmp_path, name, text + "\n")
    assert f"{name}_commands.yaml" in str(e.value), e.value


def test_configs_without_the_key_do_not_touch_the_backend(tmp_path, monkeypatch):
    """every shipped config: commands() is None and make_batched serves a backend that has no set_task_commands (the substitution seam
    envs.humanoid.BatchedEnv); a config with the block calls it, after the constructor, with the spec's keywords"""
    from learninghumanoidwalking_amd.envs import ENVIRONMENTS, humanoid

    class Plain:
        def __init__(self, model, task, n_envs, **kw):
            self.kw = kw

    class Commanded(Plain):
        def set_task_commands(self, **fields):
            self.commands = fields

    for name in ("jvrc_walk", "h1", "h1_walk", "jvrc_step", "cartpole"):
        spec = ENVIRONMENTS[name]()
        assert spec.commands() is None
        monkeypatch.setattr(humanoid, "BatchedEnv", Plain)
        env = spec.make_batched(3, seed=1)
        assert isinstance(env, Plain) and env.kw["seed"] == 1
    spec = _yaml(tmp_path, "jvrc_walk", "commands: {forward_speed_range: [0.0, 0.8]}\n")
    monkeypatch.setattr(humanoid, "BatchedEnv", Commanded)
    assert spec.make_batched(3).commands == dict(forward_vx=(0.0, 0.8)) == spec.commands()
    monkeypatch.setattr(humanoid, "BatchedEnv", Plain)
    with pytest.raises(AttributeError):
        spec.make_batched(3)      # (a config with commands needs a backend that takes them: no silent default)


def test_a_yaml_with_commands_configures_the_emulated_env(tmp_path):
    spec = _yaml(tmp_path, "jvrc_walk", "commands: {mode_probs: {standing: 0.0, inplace: 0.0, forward: 1.0}, forward_speed_range: [0.8, 0.8]}\n")
    env = BACKEND.make(spec, 2, seed=1)
    assert env.get_task_commands() == dict(C.DEFAULTS, mode_cdf=(0.0, 0.0), forward_vx=(0.8, 0.8))
    obs = C.reset(env)
    np.testing.assert_array_equal(obs[:, 31:37], np.tile(np.float32([1, 0, 0, 0, 0.8, 0]), (2, 1)))      # FORWARD at 0.8 m/s, no draw
    env.close()


# ---------------------------------------------------------------------------------------------------------------- eval --command (no library)
def _rx():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import run_experiment
    return run_experiment


def test_eval_command_spec_parses_and_spreads():
    rx = _rx()
    mode, ref = rx.parse_command("standing", 3)
    assert list(mode) == [0, 0, 0] and mode.dtype == np.int32 and not ref.any() and ref.shape == (3, 3)
    mode, ref = rx.parse_command("inplace:-0.3", 2)
    assert list(mode) == [1, 1] and ref.tolist() == [[-0.3, 0.0, 0.0]] * 2
    mode, ref = rx.parse_command("forward:0.1..0.4", 4)
    assert list(mode) == [2] * 4 and ref[:, 1].tolist() == [0.1 + k * (0.4 - 0.1) / 3 for k in range(4)] and not ref[:, [0, 2]].any()
    np.testing.assert_allclose(ref[:, 1], [0.1, 0.2, 0.3, 0.4], rtol=0, atol=1e-15)
    mode, ref = rx.parse_command("forward:0.5,-0.1..0.1", 3)
    assert ref.tolist() == [[0.0, 0.5, -0.1], [0.0, 0.5, 0.0], [0.0, 0.5, 0.1]]
    mode, ref = rx.parse_command("forward:0.1..0.4", 1)      # K = 1 gets A
    assert ref.tolist() == [[0.0, 0.1, 0.0]]
    mode, ref = rx.parse_command("inplace:0.4..-0.4", 1)
    assert ref.tolist() == [[0.4, 0.0, 0.0]]
    for bad in ("walk", "standing:1", "inplace", "inplace:0.1,0.2", "forward", "forward:1,2,3", "forward:fast", "forward:0.1..", "forward:,0.1",
                "forward:0.1..0.2..0.3", "inplace:nan", "forward:0.1..inf"):
        with pytest.raises(SystemExit) as e:
            rx.parse_command(bad, 4)
        assert "--command" in str(e.value) and repr(bad) in str(e.value), e.value


def test_first_episode_returns_are_float64_sums_in_time_order():
    rx = _rx()
    rew = np.float32([[0.1, 0.2, 0.3], [0.4, 0.5, 0.6], [0.7, 0.8, 0.9]])
    done = np.uint8([[0, 1, 0], [2, 0, 0], [0, 1, 0]])
    ret, length = rx.first_episodes(rew, done)
    assert list(length) == [2, 1, 3] and ret.dtype == np.float64
    assert ret.tolist() == [float(rew[0, 0]) + float(rew[1, 0]), float(rew[0, 1]), (float(rew[0, 2]) + float(rew[1, 2])) + float(rew[2, 2])]
