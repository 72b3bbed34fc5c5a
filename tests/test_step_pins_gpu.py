"""Pinned walk modes and footstep plans of the stepping task (lhw_env_pin_step_plans / lhw_env_get_pinned_step_plans, include/lhw.h;
BatchedEnv.pin_step_plans) on the GPU through the product BatchedEnv: the checks of tests/test_step_pins.py
(tests/step_pins_checks.py), and the history and LSTM resident rollouts through the learner.  The reference draws mode and plan inside
SteppingTask.reset (tasks/stepping_task.py:261-334)."""
import numpy as np
import pytest

from tests import step_pins_checks as C
from tests.task_shaping_checks import Backend, GpuRunner

pytestmark = pytest.mark.gpu

BACKEND = Backend(GpuRunner, device=0)


def test_a_free_env_beside_pinned_envs_and_an_unpinned_batch_change_no_bit():
    C.check_neutrality(BACKEND)


def test_pinning_what_was_drawn_is_the_identity():
    C.check_pinning_what_was_drawn_is_the_identity(BACKEND)


def test_pinned_plans_against_the_oracle():
    C.check_against_oracle(BACKEND)


def test_resident_rollout_is_bitwise_the_launch_per_step_loop_under_pins():
    C.check_resident_equals_steps(BACKEND)


def _pinned(env):
    """envs 0 and 2 hold their pinned plans, whichever reset laid them out last"""
    seq, floor, ist = env.debug_step_record()
    assert list(ist[[0, 2], 4]) == [6, 20] and list(floor[[0, 2]]) == [-2.0, -2.0]
    np.testing.assert_array_equal(seq[0, :6, 2], C.PLAN0[:, 2])
    assert set(np.round(np.diff(seq[2, :, 2]), 12)) == {0.0, C.HEIGHT2}
    return seq, floor, ist


@pytest.mark.parametrize("kind", ["history", "lstm"])
def test_history_and_lstm_resident_rollouts_are_bitwise_the_launch_per_step_loop_under_pins(kind, tmp_path, monkeypatch):
    """jvrc_step, 3 envs, through the learner: obs_history_len = 2 with T = 8 and episodes of 4 steps, or an LSTM policy with T = 4 =
    the episode length; envs 0 and 2 pinned before the first reset; two rollouts, so the second one runs on plans that resets inside the
    first launch laid out.  LHW_ROLLOUT_MODE = resident against steps, same seed: every rollout buffer, the state, the stepping record."""
    import torch
    from learninghumanoidwalking_amd.envs.jvrc_step import JvrcStepSpec
    from learninghumanoidwalking_amd.ppo import PPO
    from tests.test_rollout_history_gpu import _ppo
    from tests.test_task_commands_gpu import _args

    def run(mode):
        monkeypatch.setenv("LHW_ROLLOUT_MODE", mode)
        if kind == "history":
            algo = _ppo(tmp_path, "jvrc_step", 2, C.N, 8, seed=7, traj_len=4)
        else:
            algo = PPO(JvrcStepSpec, _args(C.N, 4, str(tmp_path / "log"), True), seed=9)
        env, ro = algo.env, algo.rollout
        C.pin_check3(env)
        out = []
        for _ in range(2):
            algo.sample_parallel_with_workers()
            assert ro.last_mode == mode, ro.last_mode
            out.append([x.clone() for x in (ro.obs, ro.act, ro.logp, ro.rew, ro.done, ro.val)])
        torch.cuda.synchronize()
        return out, env.get_state(), _pinned(env), env.pop_fault_stats()

    (a, sa, ra, fa), (b, sb, rb, fb) = run("steps"), run("resident")
    for x, y in zip(a, b):
        for n, u, v in zip(("obs", "act", "logp", "rew", "done", "val"), x, y):
            assert torch.equal(u, v), n
    np.testing.assert_array_equal(sa[0], sb[0])
    np.testing.assert_array_equal(sa[1], sb[1])
    for u, v in zip(ra, rb):
        np.testing.assert_array_equal(u, v)
    assert fa == fb
    assert (a[0][4] != 0).any(dim=0).all(), "every env must pass an auto-reset inside the first rollout"


def test_refused_calls_name_the_field_and_change_nothing_and_the_getter_round_trips():
    C.check_refusals_and_getter(BACKEND)
