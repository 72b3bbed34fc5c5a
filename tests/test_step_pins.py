"""Pinned walk modes and footstep plans of the stepping task (lhw_env_pin_step_plans / lhw_env_get_pinned_step_plans, include/lhw.h;
BatchedEnv.pin_step_plans) on the SIMT emulator: the checks of tests/step_pins_checks.py, and the history and LSTM resident rollouts
against their launch-per-step loops.  The reference draws mode and plan inside SteppingTask.reset (tasks/stepping_task.py:261-334);
what a pinned env does instead is stated by the oracle with `_generate` overridden.  CPU twin of tests/test_step_pins_gpu.py."""
import numpy as np

import torch

from tests import emu
from tests import step_pins_checks as C
from tests.task_shaping_checks import Backend, EmuRunner

BACKEND = Backend(EmuRunner, device=torch.device("cpu"), library=emu.lib)


def test_a_free_env_beside_pinned_envs_and_an_unpinned_batch_change_no_bit():
    C.check_neutrality(BACKEND)


def test_pinning_what_was_drawn_is_the_identity():
    C.check_pinning_what_was_drawn_is_the_identity(BACKEND)


def test_pinned_plans_against_the_oracle():
    C.check_against_oracle(BACKEND)


def test_resident_rollout_is_bitwise_the_launch_per_step_loop_under_pins():
    C.check_resident_equals_steps(BACKEND)


def _pinned_after_the_last_reset(env):
    """the env's record behind the auto-reset that ended the rollout: envs 0 and 2 hold their pinned plans again"""
    seq, floor, ist = env.debug_step_record()
    assert list(ist[[0, 2], 4]) == [6, 20] and list(floor[[0, 2]]) == [-2.0, -2.0]
    np.testing.assert_array_equal(seq[0, :6, 2], C.PLAN0[:, 2])
    assert set(np.round(np.diff(seq[2, :, 2]), 12)) == {0.0, C.HEIGHT2}


def test_history_resident_rollout_is_bitwise_the_launch_per_step_loop_under_pins():
    from tests import test_rollout_history as RH
    from tests.test_rollout_resident import NumpyActor
    spec, T, H = C.spec_of("jvrc_step"), 8, 2
    envs = RH._pair(spec, H, C.N, seed=7, max_traj_len=4)
    for e in envs:
        C.pin_check3(e)
    pol = NumpyActor(H * spec.obs_dim, spec.act_dim, seed=5, scale=2.0)
    obs0 = RH._first_obs(envs, H)
    a = RH._reference(envs[0], pol, T, obs0[0], H)
    b = RH._resident(envs[1], pol, T, obs0[1], H)
    RH._same(a, b)
    RH._same_state(*envs)
    assert (a["done"][:-1] != 0).any(axis=0).all(), "every env must pass an auto-reset inside the rollout"
    for e in envs:
        _pinned_after_the_last_reset(e)
    for x, y in zip(envs[0].debug_step_record(), envs[1].debug_step_record()):
        np.testing.assert_array_equal(x, y)


def test_lstm_resident_rollout_is_bitwise_the_launch_per_step_loop_under_pins():
    from tests import test_rollout_lstm as RL
    from tests.test_rollout_resident import _same
    spec, T = C.spec_of("jvrc_step"), 8
    envs, pols = RL._pair(spec, C.N, 7, 9, max_traj_len=4)
    for e in envs:
        C.pin_check3(e)
    obs0 = [e.reset().copy() for e in envs]
    reset0 = np.array([0, 1, 0], np.uint8)
    a = RL._per_step(envs[0], pols[0], T, obs0[0], reset0)
    b = RL._resident(envs[1], pols[1], T, obs0[1], reset0)
    _same(a, b)
    for x, y in zip(envs[0].get_state(), envs[1].get_state()):
        np.testing.assert_array_equal(x, y)
    RL._same_state(pols[0], pols[1])
    assert (a["done"][:-1] != 0).any(axis=0).all(), "every env must pass an auto-reset inside the rollout"
    for e in envs:
        _pinned_after_the_last_reset(e)
    for x, y in zip(envs[0].debug_step_record(), envs[1].debug_step_record()):
        np.testing.assert_array_equal(x, y)


def test_refused_calls_name_the_field_and_change_nothing_and_the_getter_round_trips():
    C.check_refusals_and_getter(BACKEND)
