"""Per-term episode statistics accumulated inside the stepping kernels (lhw_env_enable_term_stats / lhw_env_pop_term_stats), on the
SIMT emulator: jvrc_walk, an odd batch, max_traj_len short enough that every env truncates, two envs started lying on the floor so that
they terminate (and overflow the two-envs-per-wave layout: the in-wave re-run is inside), one resident rollout and the same steps
launch per step.  What the statistics stand for: the per-term `info` dictionary of the reference's env.step
(/root/reference/robots/robot_base.py:88-96), summed per episode.  CPU twin of tests/test_term_stats_gpu.py."""
import ctypes

import numpy as np
import pytest

from learninghumanoidwalking_amd._lib import LhwError
from tests import emu
from tests import term_stats_checks as C
from tests.test_rollout_resident import NumpyActor, _buffers, _fallen_states, _resident, _same

N, T1, T2, L = 5, 4, 5, 4      # N odd: the last wavefront holds one env; T = 9 control steps, every env truncates at least twice
T = T1 + T2


def _make(export):
    from learninghumanoidwalking_amd.envs.jvrc_walk import JvrcWalkSpec
    spec = JvrcWalkSpec()
    env = emu.make_emulated(spec, N, seed=3, max_traj_len=L)
    env.reset()
    q, v = _fallen_states(spec, N, seed=21)
    env.set_state(q, v)
    if export:
        C.enable(env)
    return env


def _per_step_with_terms(env, pol, T, obs0):
    """the launch-per-step pipeline of tests/test_rollout_resident.py, reading rew_terms (float32) back after every control step"""
    Lb = emu.lib()
    b = _buffers(T, env.n_envs, env.obs_dim, env.act_dim)
    b["obs"][0] = obs0
    terms = np.zeros((T, env.n_envs, env.n_terms), np.float32)
    y = np.zeros((env.n_envs, pol.view.act_pad), np.float32)
    for t in range(T):
        assert Lb.lhw_debug_policy_step(ctypes.byref(pol.view), b["obs"][t].ctypes.data, env.n_envs, 0, pol.view.counter + t, y.ctypes.data,
                                        b["act"][t].ctypes.data, b["logp"][t].ctypes.data, None) == 0
        obs, rew, done, tob = env.step(b["act"][t])
        b["obs"][t + 1], b["rew"][t], b["done"][t], b["tob"][t] = obs, rew, done, tob
        terms[t] = env.rew_terms.numpy()
    return b, terms


def test_term_stats_emulated_jvrc_walk():
    obs0 = np.zeros((N, 37), np.float32)
    pol = lambda: NumpyActor(37, 12, seed=5, scale=2.0)

    off = _make(False)                          # export off, one resident rollout
    a = _resident(off, pol(), T, obs0)
    on = _make(True)                            # export on, one resident rollout
    b = _resident(on, pol(), T, obs0)
    steps = _make(True)                         # export on, launch per step
    c, terms = _per_step_with_terms(steps, pol(), T, obs0)
    split = _make(True)                         # export on, two resident rollouts with a pop in between
    p = pol()
    d1 = _resident(split, p, T1, obs0)
    pop1, eps1 = C.pop(split), split.pop_episode_stats()
    p.view.counter += T1
    d2 = _resident(split, p, T2, d1["obs"][T1])
    pop2, eps2 = C.pop(split), split.pop_episode_stats()

    # 1. bitwise neutrality: every rollout output and the state, export on == export off, in both ways of executing a control step
    _same(a, b)
    _same(a, c)
    _same(a, {k: np.concatenate([d1[k][:T1], d2[k]]) for k in a})      # (obs: T1 slices of the first rollout, T2 + 1 of the second)
    for other in (on, steps, split):
        for x, y in zip(off.get_state(), other.get_state()):
            np.testing.assert_array_equal(x, y)
    done = a["done"]
    assert ((done & 2) != 0).any(axis=0).all(), "every env must truncate at least once"
    assert ((done & 1) != 0).any(), "no env terminated"
    reruns = on.pop_rerun_count()
    assert reruns > 0 and reruns == steps.pop_rerun_count(), "the fallen envs must take the in-wave re-run"
    assert on.pop_fault_stats() == steps.pop_fault_stats() == (0, 0)

    # 2. counts, exact
    pb, pc = C.pop(on), C.pop(steps)
    eb, ec = on.pop_episode_stats(), steps.pop_episode_stats()
    C.check_counts(pb, done, eb[2])
    C.check_counts(pc, done, ec[2])
    # 3. term sums against the host recomputation over the float32 read-backs
    host_sum, host_abs, _ = C.host_term_sums(terms, done)
    C.check_against_host(pc, host_sum, host_abs)
    C.check_against_host(pb, host_sum, host_abs)
    # 4. sum over the terms == the sum of episode returns
    C.check_same_up_to_order(pb[0].sum(), eb[0], "resident: sum of term sums vs ret_sum")
    C.check_same_up_to_order(pc[0].sum(), ec[0], "launch per step: sum of term sums vs ret_sum")
    # 5. resident == launch per step up to the order of the atomics
    C.check_same_up_to_order(pb[0], pc[0], "resident vs launch per step")
    assert pb[1:] == pc[1:]
    # 6. a second pop returns zeros; the partial sums of running episodes survive a pop
    C.check_zero(C.pop(on))
    C.check_zero(C.pop(steps))
    C.check_counts(pop1, done[:T1], eps1[2])
    C.check_counts(pop2, done[T1:], eps2[2])
    C.check_same_up_to_order(pop1[0] + pop2[0], pb[0], "two rollouts with a pop in between vs one rollout")
    h1 = C.host_term_sums(terms[:T1], done[:T1])
    h2 = C.host_term_sums(terms[T1:], done[T1:], carry=h1[2])
    C.check_against_host(pop2, h2[0], h2[1])


def test_term_stats_are_off_by_default_and_reset_with_the_env():
    env = _make(False)
    s = np.zeros(env.n_terms)
    assert env._L.lhw_env_pop_term_stats(env._h, s.ctypes.data, None, None, None) != 0
    assert b"lhw_env_enable_term_stats" in env._L.lhw_last_error()
    with pytest.raises(LhwError, match="lhw_env_enable_term_stats"):      # (the env raises with the text of its own, emulated, library)
        env.pop_term_sums()
    C.enable(env)
    act = np.zeros((N, 12), np.float32)
    env.step(act)
    env.reset()                                 # abandons the running episodes: their partial sums go with them
    for _ in range(L):
        env.step(act)
    got = C.pop(env)
    ret, _, cnt = env.pop_episode_stats()
    assert got[1] == cnt > 0
    C.check_same_up_to_order(got[0].sum(), ret, "after a reset: sum of term sums vs ret_sum")
    C.enable(env, False)                        # stops: nothing accumulates, popping is an error again
    env.step(act)
    assert env._L.lhw_env_pop_term_stats(env._h, s.ctypes.data, None, None, None) != 0


def test_term_stats_emulated_cartpole():
    from learninghumanoidwalking_amd.envs import CartpoleSpec
    env = emu.make_emulated(CartpoleSpec(), 7, seed=2, max_traj_len=6)
    ref = emu.make_emulated(CartpoleSpec(), 7, seed=2, max_traj_len=6)
    C.enable(env)
    env.reset(), ref.reset()
    Tc = 20
    tape = np.random.default_rng(0).uniform(-1, 1, size=(Tc, 7, 1)).astype(np.float32)
    terms, done = np.zeros((Tc, 7, 4), np.float32), np.zeros((Tc, 7), np.uint8)
    for t in range(Tc):
        out, want = env.step(tape[t]), ref.step(tape[t])
        for x, y in zip(out, want):
            np.testing.assert_array_equal(x, y)
        terms[t], done[t] = env.rew_terms.numpy(), env.done.numpy()
    got, eps = C.pop(env), env.pop_episode_stats()
    C.check_counts(got, done, eps[2])
    host_sum, host_abs, _ = C.host_term_sums(terms, done)
    C.check_against_host(got, host_sum, host_abs)
    C.check_same_up_to_order(got[0].sum(), eps[0], "cartpole: sum of term sums vs ret_sum")
    C.check_zero(C.pop(env))
