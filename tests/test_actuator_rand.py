"""Actuator randomisation -- PD-gain noise and back-EMF damping of the reference's RobotBase (robots/robot_base.py:5-62) as run-time
settings of the humanoid envs (lhw_env_set_actuator_randomization, include/lhw.h; `actuator_randomization:` in an env's YAML) -- on the
SIMT emulator (tests/actuator_rand_checks.py against the float64 oracle of tests/actuator_rand_oracle.py), plus the host-only parts
(YAML -> spec -> make_batched).  CPU twin of tests/test_actuator_rand_gpu.py."""
import copy
import ctypes

import numpy as np
import pytest

import torch

from tests import actuator_rand_checks as C
from tests import emu
from tests.task_shaping_checks import Backend, EmuRunner

BACKEND = Backend(EmuRunner, device=torch.device("cpu"), library=emu.lib)


def test_fresh_env_reports_the_defaults_and_setting_them_changes_no_bit():
    C.check_defaults_and_neutrality(BACKEND)


@pytest.mark.parametrize("name", ("jvrc_walk", "h1"))
def test_drawn_gains_follow_the_oracle(name):
    C.check_pdrand_parity(BACKEND, name)


@pytest.mark.parametrize("name", ("jvrc_walk", "h1"))
def test_back_emf_damping_follows_the_oracle(name):
    C.check_bemf_parity(BACKEND, name)


@pytest.mark.parametrize("name", ("jvrc_walk", "h1"))
def test_back_emf_damping_survives_resets_and_is_zeroed_when_switched_off(name):
    C.check_bemf_survives_resets(BACKEND, name)


@pytest.mark.parametrize("stats", (False, True), ids=("plain", "stats"))
@pytest.mark.parametrize("name", C.ENVS)
def test_resident_rollout_is_bitwise_the_launch_per_step_loop(name, stats):
    C.check_resident_equals_steps(BACKEND, name, stats)


def test_setter_between_two_resident_rollouts():
    C.check_setter_between_rollouts(BACKEND)


def test_clocks_and_actuator_randomisation_exclude_each_other():
    C.check_clocks_exclude(BACKEND)


def test_refused_calls_name_the_field_and_change_nothing():
    C.check_refusals(BACKEND)


def test_lstm_and_history_rollouts_are_declined_while_armed():
    """the LSTM and observation-history rollout kernels do not carry the feature: LHW_ERR_UNSUPPORTED with a message while it is armed
    (BatchedEnv returns False: the caller steps launch by launch), launched again once it is off"""
    from tests.test_rollout_lstm import NumpyLstmActor
    from tests.test_rollout_resident import NumpyActor, _buffers
    spec, T, L = C.spec_of("jvrc_walk"), 2, emu.lib()
    env = emu.make_emulated(spec, C.N, seed=2)
    pol = NumpyLstmActor(spec.obs_dim, spec.act_dim, C.N, seed=5)
    b = _buffers(T, C.N, env.obs_dim, env.act_dim)
    b["obs"][0] = env.reset()
    reset0 = np.ones(C.N, np.uint8)
    args = (pol.view, T, b["obs"], b["act"], b["logp"], b["tob"], b["rew"], b["done"], reset0)
    for kw in (dict(pdrand_k=0.1), dict(sim_bemf=True)):
        env.set_actuator_randomization(**kw)
        q0 = env.get_state()
        assert env.rollout_lstm(*args) is False
        msg = L.lhw_last_error()
        assert b"lhw_env_rollout_lstm" in msg and b"actuator randomisation" in msg, msg
        rc = L.lhw_env_rollout_lstm(env._h, ctypes.byref(pol.view), 0, C.N, T, *(x.ctypes.data for x in (b["obs"], b["act"], b["logp"], b["tob"], b["rew"], b["done"])),
                                    env.rew_terms.data_ptr(), reset0.ctypes.data, None, None, None)
        assert rc == C.ERR_UNSUPPORTED
        np.testing.assert_array_equal(env.get_state()[0], q0[0])      # nothing was launched
    env.set_actuator_randomization()
    assert env.rollout_lstm(*args) is True
    env.close()

    hspec = copy.copy(spec)
    hspec.history_len = 2
    env = emu.make_emulated(hspec, C.N, seed=2)
    pol = NumpyActor(env.obs_dim, env.act_dim, seed=5)
    b = _buffers(T, C.N, env.obs_dim, env.act_dim)
    b["obs"][0] = env.reset()
    args = (pol.view, T, b["obs"], b["act"], b["logp"], b["tob"], b["rew"], b["done"])
    env.set_actuator_randomization(pdrand_k=0.1, sim_bemf=True)
    assert env.rollout(*args) is False
    msg = L.lhw_last_error()
    assert b"lhw_env_rollout_history" in msg and b"actuator randomisation" in msg, msg
    env.set_actuator_randomization()
    assert env.rollout(*args) is True
    env.close()


# ---------------------------------------------------------------------------------------------------------------- spec / YAML (no library)
def _yaml(tmp_path, name, text):
    from learninghumanoidwalking_amd.envs import ENVIRONMENTS
    base = ENVIRONMENTS[name]().yaml_path
    path = tmp_path / f"{name}_actuator.yaml"
    path.write_text(f"inherits: {base}\n" + text)      # (load_config: the child's keys win; an absolute parent path is taken as it is)
    return ENVIRONMENTS[name](yaml_path=str(path))


def test_yaml_key_gives_the_setter_keywords(tmp_path):
    spec = _yaml(tmp_path, "jvrc_walk", "actuator_randomization: {pdrand_k: 0.1, sim_bemf: true}\n")
    assert spec.actuator_randomization() == dict(pdrand_k=0.1, sim_bemf=True, bemf_range=(5.0, 40.0), bemf_interval=10)
    assert "actuator_randomization" not in spec.env_args()[2]      # (a setting of the env, not of its creation)
    spec = _yaml(tmp_path, "h1", "actuator_randomization: {sim_bemf: true, bemf_range: [2, 20], bemf_interval: 4, sim_motor_dyn: false}\n")
    assert spec.actuator_randomization() == dict(pdrand_k=0.0, sim_bemf=True, bemf_range=(2.0, 20.0), bemf_interval=4)
    assert _yaml(tmp_path, "jvrc_step", "actuator_randomization: {}\n").actuator_randomization() == C.DEFAULTS


def test_yaml_mistakes_are_refused(tmp_path):
    with pytest.raises(KeyError) as e:
        _yaml(tmp_path, "jvrc_walk", "actuator_randomization: {pdrand: 0.1}\n")
    assert all(k in str(e.value) for k in ("pdrand_k", "sim_bemf", "bemf_range", "bemf_interval"))      # (names the valid keys)
    with pytest.raises(NotImplementedError) as e:
        _yaml(tmp_path, "jvrc_walk", "actuator_randomization: {sim_motor_dyn: true}\n")
    assert "sim_motor_dyn" in str(e.value)
    for text in ("{pdrand_k: 1.0}", "{pdrand_k: -0.1}", "{bemf_range: [10, 5]}", "{bemf_range: [-1, 5]}", "{bemf_interval: 0}"):
        with pytest.raises(ValueError):
            _yaml(tmp_path, "jvrc_walk", f"actuator_randomization: {text}\n")


def test_configs_without_the_key_do_not_touch_the_backend(tmp_path, monkeypatch):
    """every shipped config: actuator_randomization() is None and make_batched serves a backend that has no setter (the substitution seam
    envs.humanoid.BatchedEnv); a config with the key calls it, after the constructor, with the spec's keywords"""
    from learninghumanoidwalking_amd.envs import ENVIRONMENTS, humanoid

    class Plain:
        def __init__(self, model, task, n_envs, **kw):
            self.kw = kw

    class Randomised(Plain):
        def set_actuator_randomization(self, **kw):
            self.actuator = kw

    for name in C.ENVS + ("cartpole",):
        spec = ENVIRONMENTS[name]()
        assert spec.actuator_randomization() is None
        monkeypatch.setattr(humanoid, "BatchedEnv", Plain)
        env = spec.make_batched(3, seed=1)
        assert isinstance(env, Plain) and env.kw["seed"] == 1
    spec = _yaml(tmp_path, "jvrc_walk", "actuator_randomization: {pdrand_k: 0.1, sim_bemf: true}\n")
    monkeypatch.setattr(humanoid, "BatchedEnv", Randomised)
    assert spec.make_batched(3).actuator == spec.actuator_randomization()
    monkeypatch.setattr(humanoid, "BatchedEnv", Plain)
    with pytest.raises(AttributeError):
        spec.make_batched(3)      # (such a config needs a backend that can randomise: no silent default)


def test_make_batched_applies_the_yaml_key_to_the_env(tmp_path):
    spec = _yaml(tmp_path, "jvrc_walk", "actuator_randomization: {pdrand_k: 0.15, sim_bemf: true, bemf_interval: 3}\n")
    env = emu.make_emulated(spec, 2, seed=1)
    assert env.actuator_randomization == dict(pdrand_k=0.15, sim_bemf=True, bemf_range=(5.0, 40.0), bemf_interval=3)
    env.close()
