"""The resident rollout for LSTM actors (lhw_env_rollout_lstm: the in-wave recurrent policy step + the control step for T control steps
in one launch, csrc/lhw_humanoid_rollout.hip) against the launch-per-step pipeline (T x { lhw_debug_lstm_policy_step ; control-step
launch }), on the SIMT emulator: every buffer of the rollout must be BITWISE the same -- observations, actions, log-densities, terminal
observations, rewards, done flags, the env state and the four LSTM state arrays afterwards.  Reference semantics: RolloutWorker.sample
with a recurrent policy, /root/reference/rl/workers/rollout_worker.py:130-190 (hidden state carried from step to step, zeroed where an
episode starts).  CPU twin of tests/test_rollout_lstm_gpu.py."""
import ctypes

import numpy as np
import pytest

from tests import emu
from tests.test_rollout_resident import _buffers, _fallen_states, _same

H = 256


class NumpyLstmActor:
    """A random float32 LSTM actor obs -> LSTMCell 256 -> LSTMCell 256 -> act as the LhwRolloutLstmPolicy view, weights and state in host
    arrays (the emulated library reads and writes them).  The state sits in buffers shaped like an LhwRnn handle's: h1 behind the
    observation columns of the [N][obs_pad + 256] step input of cell 1, h2 in the upper half of cell 2's [N][512] input."""

    def __init__(self, obs_dim, act_dim, n_rows, seed, scale=1.0, deterministic=False, counter=7):
        from learninghumanoidwalking_amd import _lib as product
        rs = np.random.default_rng(seed)
        Dp, Op = (obs_dim + 3) // 4 * 4, (act_dim + 3) // 4 * 4
        K1 = Dp + H
        w1 = np.zeros((4 * H, K1), np.float32)
        w1[:, :obs_dim] = rs.normal(size=(4 * H, obs_dim)) * scale / np.sqrt(obs_dim)
        w1[:, Dp:] = rs.normal(size=(4 * H, H)) * scale / np.sqrt(H)
        w2 = (rs.normal(size=(4 * H, 2 * H)) * scale / np.sqrt(H)).astype(np.float32)
        wo = np.zeros((Op, H), np.float32)
        wo[:act_dim] = rs.normal(size=(act_dim, H)) * 2.0 * scale / np.sqrt(H)
        bias = lambda: (rs.normal(size=4 * H) * 0.1).astype(np.float32)
        self.a = dict(w1t=np.ascontiguousarray(w1.T), bi1=bias(), bh1=bias(), w2t=np.ascontiguousarray(w2.T), bi2=bias(), bh2=bias(),
                      wot=np.ascontiguousarray(wo.T), bo=np.zeros(Op, np.float32), stdv=np.full(act_dim, 0.223, np.float32),
                      obs_mean=(rs.normal(size=obs_dim) * 0.1).astype(np.float32), obs_std=(0.5 + rs.uniform(size=obs_dim)).astype(np.float32))
        self.a["bo"][:act_dim] = rs.normal(size=act_dim) * 0.05
        # a state that is not zero, so that reset0 decides something
        self.xh1 = (rs.uniform(-0.5, 0.5, size=(n_rows, K1))).astype(np.float32)
        self.xh2 = (rs.uniform(-0.5, 0.5, size=(n_rows, 2 * H))).astype(np.float32)
        self.c1 = (rs.normal(size=(n_rows, H)) * 0.5).astype(np.float32)
        self.c2 = (rs.normal(size=(n_rows, H)) * 0.5).astype(np.float32)
        self.Dp = Dp
        q = product.LhwRolloutLstmPolicy()
        for k, v in self.a.items():
            setattr(q, k, v.ctypes.data)
        q.h1, q.h1_ld = self.xh1.ctypes.data + 4 * Dp, K1
        q.h2, q.h2_ld = self.xh2.ctypes.data + 4 * H, 2 * H
        q.c1, q.c2, q.state_rows = self.c1.ctypes.data, self.c2.ctypes.data, n_rows
        q.obs_dim, q.obs_pad, q.act_dim, q.act_pad, q.hidden = obs_dim, Dp, act_dim, Op, H
        q.deterministic, q.seed, q.counter = int(deterministic), 1234567, counter
        self.view = q

    def state(self):
        return dict(h1=self.xh1[:, self.Dp:].copy(), h2=self.xh2[:, H:].copy(), c1=self.c1.copy(), c2=self.c2.copy())


def _per_step(env, pol, T, obs0, reset0):
    """the launch-per-step pipeline: the reference policy launch, then the control-step launch(es); the episode-start mask of step t is
    reset0 at t = 0 and done[t - 1] != 0 afterwards (what RecurrentRollout hands lhw_rnn_forward)"""
    L = emu.lib()
    N, D, A = env.n_envs, env.obs_dim, env.act_dim
    b = _buffers(T, N, D, A)
    b["obs"][0] = obs0
    y = np.zeros((N, pol.view.act_pad), np.float32)
    reset = np.ascontiguousarray(reset0, np.uint8)
    for t in range(T):
        rc = L.lhw_debug_lstm_policy_step(ctypes.byref(pol.view), b["obs"][t].ctypes.data, N, reset.ctypes.data, 0, pol.view.counter + t,
                                          y.ctypes.data, b["act"][t].ctypes.data, b["logp"][t].ctypes.data, None)
        assert rc == 0, L.lhw_last_error()
        obs, rew, done, tob = env.step(b["act"][t])
        b["obs"][t + 1], b["rew"][t], b["done"][t], b["tob"][t] = obs, rew, done, tob
        reset = (done != 0).astype(np.uint8)
    return b


def _resident(env, pol, T, obs0, reset0, first=0, count=None):
    b = _buffers(T, env.n_envs, env.obs_dim, env.act_dim)
    b["obs"][0] = obs0
    assert env.rollout_lstm(pol.view, T, b["obs"], b["act"], b["logp"], b["tob"], b["rew"], b["done"], np.ascontiguousarray(reset0, np.uint8),
                            first=first, count=count)
    return b


def _same_state(pa, pb, rows=slice(None)):
    sa, sb = pa.state(), pb.state()
    for k in sa:
        np.testing.assert_array_equal(sa[k][rows], sb[k][rows], err_msg=k)


def _spec(name):
    if name == "jvrc_walk":
        from learninghumanoidwalking_amd.envs.jvrc_walk import JvrcWalkSpec as S
    elif name == "h1":
        from learninghumanoidwalking_amd.envs.h1 import H1Spec as S
    elif name == "h1_walk":
        from learninghumanoidwalking_amd.envs.h1_walk import H1WalkSpec as S
    else:
        from learninghumanoidwalking_amd.envs.jvrc_step import JvrcStepSpec as S
    return S()


def _pair(spec, N, seed, pol_seed, **kw):
    envs = [emu.make_emulated(spec, N, seed=seed, **kw) for _ in range(2)]
    pols = [NumpyLstmActor(spec.obs_dim, spec.act_dim, N, seed=pol_seed, scale=2.0) for _ in range(2)]
    return envs, pols


def test_lstm_resident_rollout_is_bitwise_the_launch_per_step_rollout_jvrc_walk():
    spec = _spec("jvrc_walk")
    N, T = 5, 7                                   # odd: the last wavefront holds one env
    envs, pols = _pair(spec, N, 3, 5, max_traj_len=4)      # truncation + auto-reset, hence state resets, inside the rollout
    obs0 = [e.reset().copy() for e in envs]
    reset0 = np.array([1, 0, 1, 1, 0], np.uint8)
    a = _per_step(envs[0], pols[0], T, obs0[0], reset0)
    b = _resident(envs[1], pols[1], T, obs0[1], reset0)
    _same(a, b)
    assert a["done"][:-1].any(), "no episode end, hence no state reset, inside the rollout"
    for x, y in zip(envs[0].get_state(), envs[1].get_state()):
        np.testing.assert_array_equal(x, y)
    _same_state(pols[0], pols[1])
    assert envs[0].pop_episode_stats() == envs[1].pop_episode_stats()
    # reset0 decides something: with another mask the first actions differ
    envs2, pols2 = _pair(spec, N, 3, 5, max_traj_len=4)
    c = _resident(envs2[0], pols2[0], 1, envs2[0].reset().copy(), 1 - reset0)
    assert not np.array_equal(c["act"][0], b["act"][0])
    # a second rollout continues from the first one's last observation, counters, flags and LSTM state
    for p in pols:
        p.view.counter += T
    r0 = (a["done"][T - 1] != 0).astype(np.uint8)
    a2 = _per_step(envs[0], pols[0], 3, a["obs"][T], r0)
    b2 = _resident(envs[1], pols[1], 3, b["obs"][T], r0)
    _same(a2, b2)
    _same_state(pols[0], pols[1])


def test_lstm_resident_rollout_repeats_overflowing_envs_inside_the_wave():
    spec = _spec("jvrc_walk")
    N, T = 4, 4
    envs, pols = _pair(spec, N, 11, 8, max_traj_len=50)
    q, v = _fallen_states(spec, N, seed=21)
    for e in envs:
        e.reset()
        e.set_state(q, v)
    obs0 = envs[0].obs.numpy().copy()
    reset0 = np.ones(N, np.uint8)
    a = _per_step(envs[0], pols[0], T, obs0, reset0)
    b = _resident(envs[1], pols[1], T, obs0, reset0)
    _same(a, b)
    ra, rb = envs[0].pop_rerun_count(), envs[1].pop_rerun_count()
    assert ra > 0 and ra == rb, (ra, rb)
    for x, y in zip(envs[0].get_state(), envs[1].get_state()):
        np.testing.assert_array_equal(x, y)
    _same_state(pols[0], pols[1])


def test_lstm_resident_rollout_of_a_sub_range_leaves_the_other_envs_and_their_state_alone():
    spec = _spec("jvrc_walk")
    N, T = 5, 3
    envs, pols = _pair(spec, N, 4, 6, max_traj_len=0)
    before = pols[1].state()
    obs0 = [e.reset().copy() for e in envs]
    reset0 = np.array([0, 1, 0, 0, 1], np.uint8)
    a = _per_step(envs[0], pols[0], T, obs0[0], reset0)
    b = _resident(envs[1], pols[1], T, obs0[1], reset0, first=1, count=3)      # envs 1..3: an odd range that starts inside a wavefront pair
    _same(a, b, rows=slice(1, 4))
    assert not b["act"][:, [0, 4]].any() and not b["obs"][1:, [0, 4]].any()
    _same_state(pols[0], pols[1], rows=slice(1, 4))
    after = pols[1].state()
    for k in before:
        np.testing.assert_array_equal(before[k][[0, 4]], after[k][[0, 4]], err_msg=k)


@pytest.mark.parametrize("name", ["h1", "h1_walk", "jvrc_step"])
def test_lstm_resident_rollout_other_tasks(name):
    spec = _spec(name)
    N, T = 3, 5
    envs, pols = _pair(spec, N, 2, 9, max_traj_len=3)
    obs0 = [e.reset().copy() for e in envs]
    reset0 = np.array([0, 1, 0], np.uint8)
    a = _per_step(envs[0], pols[0], T, obs0[0], reset0)
    b = _resident(envs[1], pols[1], T, obs0[1], reset0)
    _same(a, b)
    assert a["done"][:-1].any()
    for x, y in zip(envs[0].get_state(), envs[1].get_state()):
        np.testing.assert_array_equal(x, y)
    _same_state(pols[0], pols[1])


def test_lstm_resident_rollout_through_the_job_queue_is_bitwise_the_same(monkeypatch):
    """jvrc_step with more env groups than wave slots (forced by LHW_ROLLOUT_SLOTS): a group's chunks run on whichever wave is free, and
    the LSTM state travels through the view's HBM buffers from one wave to the next."""
    spec = _spec("jvrc_step")
    N, T = 4, 7
    envs = [emu.make_emulated(spec, N, seed=3, max_traj_len=4) for _ in range(3)]
    pols = [NumpyLstmActor(spec.obs_dim, spec.act_dim, N, seed=5, scale=2.0) for _ in range(3)]
    obs0 = [e.reset().copy() for e in envs]
    reset0 = np.array([1, 0, 0, 1], np.uint8)
    a = _per_step(envs[0], pols[0], T, obs0[0], reset0)
    monkeypatch.setenv("LHW_ROLLOUT_CHUNK", "0")
    b = _resident(envs[1], pols[1], T, obs0[1], reset0)
    monkeypatch.setenv("LHW_ROLLOUT_CHUNK", "3")
    monkeypatch.setenv("LHW_ROLLOUT_SLOTS", "1")
    c = _resident(envs[2], pols[2], T, obs0[2], reset0)
    assert envs[2].last_rollout_queued() and not envs[1].last_rollout_queued()
    _same(a, b)
    _same(a, c)
    assert a["done"][:-1].any()
    for e in envs[1:]:
        for x, y in zip(envs[0].get_state(), e.get_state()):
            np.testing.assert_array_equal(x, y)
    _same_state(pols[0], pols[1])
    _same_state(pols[0], pols[2])


@pytest.mark.parametrize("name", ["jvrc_walk", "jvrc_step", "h1", "h1_walk", "jvrc_step_queued"])
def test_lstm_resident_rollout_with_armed_term_statistics_gives_the_same_bits(name, monkeypatch):
    queued = name.endswith("_queued")
    spec = _spec(name[:-7] if queued else name)
    N, T, traj = (3, 5, 3) if name in ("jvrc_walk", "jvrc_step") else (3, 2, 2)      # (the later cases: one auto-reset, on the last step)
    if queued:      # every (group, control step) a job of one resident wave
        monkeypatch.setenv("LHW_ROLLOUT_CHUNK", "1")
        monkeypatch.setenv("LHW_ROLLOUT_SLOTS", "1")
    envs, pols = _pair(spec, N, 6, 4, max_traj_len=traj)
    envs[1].enable_term_stats()
    obs0 = [e.reset().copy() for e in envs]
    reset0 = np.ones(N, np.uint8)
    a = _resident(envs[0], pols[0], T, obs0[0], reset0)
    b = _resident(envs[1], pols[1], T, obs0[1], reset0)
    _same(a, b)
    _same_state(pols[0], pols[1])
    assert all(e.last_rollout_queued() == queued for e in envs)
    from tests import term_stats_checks as C
    assert C.pop(envs[1])[1] == int((a["done"] != 0).sum()) > 0


def test_lstm_rollout_refuses_what_the_lane_mapping_does_not_cover():
    spec = _spec("jvrc_walk")
    env = emu.make_emulated(spec, 2, seed=1, max_traj_len=0)
    pol = NumpyLstmActor(spec.obs_dim, spec.act_dim, 2, seed=1)
    obs0 = env.reset().copy()
    L = emu.lib()
    b = _buffers(1, 2, env.obs_dim, env.act_dim)
    b["obs"][0] = obs0
    r0 = np.zeros(2, np.uint8)
    args = lambda: (env._h, ctypes.byref(pol.view), 0, 2, 1, b["obs"].ctypes.data, b["act"].ctypes.data, b["logp"].ctypes.data, b["tob"].ctypes.data,
                    b["rew"].ctypes.data, b["done"].ctypes.data, env.rew_terms.data_ptr(), r0.ctypes.data, None, None, None)
    pol.view.hidden = 32
    assert L.lhw_env_rollout_lstm(*args()) == -4      # LHW_ERR_UNSUPPORTED
    pol.view.hidden = 256
    pol.view.state_rows = 1                           # fewer state rows than envs
    assert L.lhw_env_rollout_lstm(*args()) == -4
    pol.view.state_rows = 2
    assert L.lhw_env_rollout_lstm(*args()) == 0
