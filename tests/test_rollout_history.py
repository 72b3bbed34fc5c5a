"""The resident rollout of an env with an observation history (lhw_env_rollout_history, obs_history_len > 1 of the reference's YAML
configs: envs/common/base_humanoid_env.py:53,177-197,274) on the SIMT emulator, against a loop of { lhw_debug_policy_step on the
H x base wide rows ; env.step ; the history rule in numpy }: every buffer BITWISE the same -- observations, actions, log-densities,
rewards, done flags, the terminal rows where an episode ended -- and the env state and episode statistics afterwards.
CPU twin of tests/test_rollout_history_gpu.py."""
import copy
import ctypes

import numpy as np
import pytest

from tests import emu
from tests.test_rollout_resident import NumpyActor, _buffers, _fallen_states

def _first_full(base_obs, H):
    """the full observation after a reset: the base observation in front of an emptied, zero-filled history"""
    full = np.zeros((base_obs.shape[0], H * base_obs.shape[1]), np.float32)
    full[:, :base_obs.shape[1]] = base_obs
    return full


def _history_env(spec, H, N, **kw):
    """the emulated BatchedEnv of `spec` with history_len = H (make_batched takes the length from the spec)"""
    spec = copy.copy(spec)
    spec.history_len = H
    env = emu.make_emulated(spec, N, **kw)
    assert env.history_len == H and env.obs_dim == H * env.base_obs_dim
    return env


def _pair(spec, H, N, **kw):
    """(a plain env for the launch-per-step reference, its twin with the history for the resident rollout)"""
    return [emu.make_emulated(spec, N, **kw), _history_env(spec, H, N, **kw)]


def _reference(env, pol, T, obs0, H):
    """launch per step: the policy launch on the full rows, the control step, batched_env.history_update's rule"""
    L = emu.lib()
    N, B, A = env.n_envs, env.obs_dim, env.act_dim
    D = H * B
    b = _buffers(T, N, D, A)
    b["obs"][0] = obs0
    y = np.zeros((N, pol.view.act_pad), np.float32)
    for t in range(T):
        rc = L.lhw_debug_policy_step(ctypes.byref(pol.view), b["obs"][t].ctypes.data, N, 0, pol.view.counter + t, y.ctypes.data,
                                     b["act"][t].ctypes.data, b["logp"][t].ctypes.data, None)
        assert rc == 0, L.lhw_last_error()
        obs, rew, done, tob = env.step(b["act"][t])
        tail = b["obs"][t][:, :D - B]
        b["obs"][t + 1] = np.concatenate([obs, np.where(done[:, None] != 0, np.float32(0), tail)], axis=1)
        b["tob"][t] = np.concatenate([tob, tail], axis=1)
        b["rew"][t], b["done"][t] = rew, done
    return b


def _resident(env, pol, T, obs0, H, first=0, count=None, launched=True):
    """BatchedEnv.rollout of an env built with history_len = H (lhw_env_rollout_history); `launched`: False where the library declines"""
    assert env.history_len == H
    b = _buffers(T, env.n_envs, env.obs_dim, env.act_dim)
    b["obs"][0] = obs0
    ok = env.rollout(pol.view, T, b["obs"], b["act"], b["logp"], b["tob"], b["rew"], b["done"], first=first, count=count)
    assert ok == launched, emu.lib().lhw_last_error()
    return b


def _first_obs(envs, H):
    """reset (plain env, history env): the hand-built first full observation of the former, which the latter's reset must return"""
    want, got = _first_full(envs[0].reset(), H), envs[1].reset().copy()
    np.testing.assert_array_equal(want, got)
    return [want, got]


def _same(a, b, rows=slice(None)):
    for k in ("obs", "act", "logp", "rew", "done"):
        np.testing.assert_array_equal(a[k][:, rows], b[k][:, rows], err_msg=k)
    ended = a["done"][:, rows] != 0
    np.testing.assert_array_equal(a["tob"][:, rows][ended], b["tob"][:, rows][ended], err_msg="tob")


def _same_state(e0, e1):
    for x, y in zip(e0.get_state(), e1.get_state()):
        np.testing.assert_array_equal(x, y)


def test_history_rollout_is_bitwise_the_launch_per_step_loop_jvrc_walk():
    from learninghumanoidwalking_amd.envs.jvrc_walk import JvrcWalkSpec
    spec = JvrcWalkSpec()
    N, T, H = 5, 7, 3                             # odd: the last wavefront holds one env
    envs = _pair(spec, H, N, seed=3, max_traj_len=4)     # truncation + auto-reset inside the rollout
    pol = NumpyActor(H * 37, 12, seed=5, scale=2.0)
    obs0 = _first_obs(envs, H)
    a = _reference(envs[0], pol, T, obs0[0], H)
    b = _resident(envs[1], pol, T, obs0[1], H)
    _same(a, b)
    assert (a["done"] & 2).any(), "no truncation / auto-reset inside the rollout"
    # the history is zero exactly behind an episode end (a live row's older entries are normalised joint states: never all zero)
    for t in range(T):
        np.testing.assert_array_equal((b["obs"][t + 1][:, 37:] == 0).all(axis=1), b["done"][t] != 0)
        assert not np.signbit(b["obs"][t + 1][b["done"][t] != 0][:, 37:]).any()      # +0
    _same_state(*envs)
    assert envs[0].pop_episode_stats() == envs[1].pop_episode_stats()
    # a second rollout continues from the first one's last observation and counters
    pol.view.counter += T
    a2 = _reference(envs[0], pol, 3, a["obs"][T], H)
    b2 = _resident(envs[1], pol, 3, b["obs"][T], H)
    _same(a2, b2)
    _same_state(*envs)


def test_history_shift_follows_the_in_wave_rerun_of_an_overflowing_env():
    from learninghumanoidwalking_amd.envs.jvrc_walk import JvrcWalkSpec
    spec = JvrcWalkSpec()
    N, T, H = 4, 4, 2
    envs = _pair(spec, H, N, seed=11, max_traj_len=50)
    pol = NumpyActor(H * 37, 12, seed=8)
    q, v = _fallen_states(spec, N, seed=21)
    for e in envs:
        e.reset()
        e.set_state(q, v)
    obs0 = _first_full(envs[0].obs.numpy(), H)      # (the observation still describes the reset pose: the same stale input for both paths)
    a = _reference(envs[0], pol, T, obs0, H)
    b = _resident(envs[1], pol, T, obs0, H)
    _same(a, b)
    ra, rb = envs[0].pop_rerun_count(), envs[1].pop_rerun_count()
    assert ra > 0 and ra == rb, (ra, rb)
    assert envs[0].pop_fault_stats() == envs[1].pop_fault_stats() == (0, 0)
    _same_state(*envs)


def test_history_rollout_of_a_sub_range_leaves_the_other_envs_alone():
    from learninghumanoidwalking_amd.envs.jvrc_walk import JvrcWalkSpec
    spec = JvrcWalkSpec()
    N, T, H = 5, 3, 2
    envs = _pair(spec, H, N, seed=4, max_traj_len=2)
    pol = NumpyActor(H * 37, 12, seed=6, deterministic=True)
    obs0 = _first_obs(envs, H)
    a = _reference(envs[0], pol, T, obs0[0], H)
    b = _resident(envs[1], pol, T, obs0[1], H, first=1, count=3)      # envs 1..3: an odd range that starts inside a wavefront pair
    _same(a, b, rows=slice(1, 4))
    for k in ("act", "logp", "tob", "rew", "done"):
        assert not b[k][:, [0, 4]].any(), k
    assert not b["obs"][1:, [0, 4]].any()
    qa, qb = envs[0].get_state()[0], envs[1].get_state()[0]
    np.testing.assert_array_equal(qa[1:4], qb[1:4])
    assert not np.array_equal(qa[0], qb[0])


def test_history_rollout_h1_keeps_the_observation_noise_counter():
    """h1 draws its observation noise from a per-env counter that advances with every observation written: the base rows the kernel
    stages for the history are the ONLY observations it writes, so the draws stay those of the launch-per-step loop"""
    from learninghumanoidwalking_amd.envs.h1 import H1Spec
    spec = H1Spec()
    N, T, H = 3, 5, 2
    envs = _pair(spec, H, N, seed=2, max_traj_len=3)
    pol = NumpyActor(H * spec.obs_dim, spec.act_dim, seed=9)
    obs0 = _first_obs(envs, H)
    a = _reference(envs[0], pol, T, obs0[0], H)
    b = _resident(envs[1], pol, T, obs0[1], H)
    _same(a, b)
    assert (a["done"] != 0).any()
    _same_state(*envs)
    # one more launch-per-step control step on both: the next observation (and its noise draw) is the same
    # (the history env continues from the rollout's last observation: its older entries, emptied where this step ends an episode)
    act = np.zeros((N, spec.act_dim), np.float32)
    base, _, done, _ = envs[0].step(act)
    tail = np.where(done[:, None] != 0, np.float32(0), a["obs"][T][:, :(H - 1) * spec.obs_dim])
    np.testing.assert_array_equal(np.concatenate([base, tail], axis=1), envs[1].step(act)[0])


def test_history_rollout_through_the_job_queue(monkeypatch):
    from learninghumanoidwalking_amd.envs.jvrc_step import JvrcStepSpec
    spec = JvrcStepSpec()
    N, T, H = 3, 7, 2
    envs = _pair(spec, H, N, seed=3, max_traj_len=4)
    pol = NumpyActor(H * spec.obs_dim, spec.act_dim, seed=5, scale=2.0)
    obs0 = _first_obs(envs, H)
    a = _reference(envs[0], pol, T, obs0[0], H)
    monkeypatch.setenv("LHW_ROLLOUT_CHUNK", "3")      # a chunk that does not divide T
    monkeypatch.setenv("LHW_ROLLOUT_SLOTS", "1")      # one resident wave drains every (group, chunk) job
    b = _resident(envs[1], pol, T, obs0[1], H)
    assert envs[1].last_rollout_queued()
    _same(a, b)
    assert (a["done"] & 2).any()
    _same_state(*envs)
    assert envs[0].pop_episode_stats() == envs[1].pop_episode_stats()


@pytest.mark.parametrize("name,stats", [("h1_walk", False), ("jvrc_step", False), ("jvrc_walk", True), ("h1", True), ("h1_walk", True), ("jvrc_step", True),
                                        ("jvrc_step_queued", True)])
def test_history_rollout_other_kernels(name, stats, monkeypatch):
    """the history kernels no test above launches: the remaining tasks against the launch-per-step loop, and the kernels that keep the
    per-term episode statistics (lhw_env_enable_term_stats) against their plain twins -- the same bits; one auto-reset (on the last step) inside"""
    from tests.test_rollout_lstm import _spec
    queued = name.endswith("_queued")
    spec = _spec(name[:-7] if queued else name)
    N, T, H = 3, 2, 2
    envs = [_history_env(spec, H, N, seed=3, max_traj_len=2) for _ in range(2)] if stats else _pair(spec, H, N, seed=3, max_traj_len=2)
    pol = NumpyActor(H * spec.obs_dim, spec.act_dim, seed=5, scale=2.0)
    obs0 = [e.reset().copy() for e in envs] if stats else _first_obs(envs, H)
    if stats:
        envs[1].enable_term_stats()
    if queued:      # every (group, control step) a job of one resident wave
        monkeypatch.setenv("LHW_ROLLOUT_CHUNK", "1")
        monkeypatch.setenv("LHW_ROLLOUT_SLOTS", "1")
    a = _resident(envs[0], pol, T, obs0[0], H) if stats else _reference(envs[0], pol, T, obs0[0], H)
    b = _resident(envs[1], pol, T, obs0[1], H)
    _same(a, b)
    assert envs[1].last_rollout_queued() == queued
    assert (a["done"] != 0).any()
    _same_state(*envs)
    if stats:
        from tests import term_stats_checks as C
        assert C.pop(envs[1])[1] == int((a["done"] != 0).sum())


def test_history_entry_point_bounds_and_history_one():
    from learninghumanoidwalking_amd import _lib as product
    from learninghumanoidwalking_amd.envs.jvrc_walk import JvrcWalkSpec
    spec = JvrcWalkSpec()
    N, T = 3, 2
    # history_len = 1 with a row padded to the strip kernels' full 64 columns: the kernels and the bits of lhw_env_rollout
    pol = NumpyActor(37, 12, seed=12)
    w1t = np.zeros((64, 256), np.float32)
    w1t[:40] = pol.a["w1t"]
    pol.a["w1t"] = w1t
    pol.view.w1t, pol.view.obs_pad = w1t.ctypes.data, 64
    envs = [emu.make_emulated(spec, N, seed=6, max_traj_len=0) for _ in range(2)]
    obs0 = [e.reset().copy() for e in envs]
    a = _buffers(T, N, 37, 12)
    a["obs"][0] = obs0[0]
    assert envs[0].rollout(pol.view, T, a["obs"], a["act"], a["logp"], a["tob"], a["rew"], a["done"])
    # (the entry point itself with history_len = 1: BatchedEnv.rollout takes lhw_env_rollout for such an env)
    L, env = emu.lib(), envs[1]
    b = _buffers(T, N, 37, 12)
    b["obs"][0] = obs0[1]
    rc = L.lhw_env_rollout_history(env._h, ctypes.byref(pol.view), 0, N, T, 1, *(ctypes.c_void_p(b[k].ctypes.data) for k in ("obs", "act", "logp", "tob", "rew", "done")),
                                   ctypes.c_void_p(env.rew_terms.data_ptr()), None, None, None)
    assert rc == 0, (rc, L.lhw_last_error())
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    _same_state(*envs)
    # the policy's width must be history_len x the env's, and within the capacity of the in-wave step
    cap = product.ROLLOUT_HISTORY_MAX_OBS_PAD
    H = cap // 37                                 # the longest history whose padded row fits: 6 x 37 = 222 -> 224
    assert (H + 1) * 37 > cap
    for h, width in ((H + 1, H + 1), (2, 3)):      # past the capacity; a policy of another width
        env = _history_env(spec, h, N, seed=6, max_traj_len=0)
        _resident(env, NumpyActor(width * 37, 12, seed=1), 1, env.reset().copy(), h, launched=False)      # (LHW_ERR_UNSUPPORTED)
    # ... at the capacity, and with fp16 operands, the in-wave step is still the reference launch bit for bit
    for half in (0, 1):
        twins = _pair(spec, H, N, seed=7, max_traj_len=0)
        wide = NumpyActor(H * 37, 12, seed=13, scale=1.5)
        wide.view.fp16_operands = half
        full = _first_obs(twins, H)
        rs = np.random.default_rng(3)
        full[0][:, 37:] = full[1][:, 37:] = rs.normal(size=(N, (H - 1) * 37)).astype(np.float32)      # a filled history
        _same(_reference(twins[0], wide, 2, full[0], H), _resident(twins[1], wide, 2, full[1], H))
