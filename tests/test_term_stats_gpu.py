"""Per-term episode statistics accumulated inside the stepping kernels (lhw_env_enable_term_stats / lhw_env_pop_term_stats) on the GPU:
the checks of tests/test_term_stats.py for every task, in every way a control step is executed -- launch per step, the resident
rollout, the job queue, the in-wave re-run -- plus one leg against the float64 oracle.  What the statistics stand for: the per-term
`info` dictionary of the reference's env.step (/root/reference/robots/robot_base.py:88-96), summed per episode."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import term_stats_checks as C

pytestmark = pytest.mark.gpu

T1 = 12      # control steps per rollout = max_traj_len: every env truncates in the first of a run's two rollouts at the latest


def _args(N, T, recurrent=False):
    return SimpleNamespace(gamma=0.99, lam=0.95, lr=3e-4, eps=1e-5, entropy_coeff=0.0, clip=0.2, minibatch_size=512, epochs=1,
                           max_traj_len=T, num_procs=N, num_envs=N, max_grad_norm=0.5, mirror_coeff=0.4, eval_freq=10**9,
                           recurrent=recurrent, imitate=None, learn_std=False, std_dev=0.4, no_mirror=True, continued=None,
                           logdir="/tmp/lhw_test_term_stats", device_index=0)


def _run(env_name, N, mode, export, monkeypatch, prepare=None, pop_between=False):
    """Two rollouts of T1 control steps each with a fresh learner (episodes carry over from the first into the second).  Returns the
    rollout buffers, the per-step reward terms (launch-per-step mode only), the state, and the popped statistics."""
    from learninghumanoidwalking_amd.envs import ENVIRONMENTS
    from learninghumanoidwalking_amd.ppo import PPO
    monkeypatch.setenv("LHW_ROLLOUT_MODE", mode)
    algo = PPO(ENVIRONMENTS[env_name], _args(N, T1), seed=9, term_stats=export)
    env, ro = algo.env, algo.rollout
    if prepare is not None:
        prepare(algo)
    terms = []
    if mode == "steps":
        orig = env.step

        def step(*a, **k):
            r = orig(*a, **k)
            terms.append(env.rew_terms.cpu().numpy().copy())
            return r

        env.step = step
    bufs, pops, eps = [], [], []
    for i in range(2):
        ro.collect()
        assert ro.last_mode == mode
        bufs.append([x.cpu().numpy().copy() for x in (ro.obs, ro.act, ro.logp, ro.tob_all, ro.rew, ro.done)])
        if export and (pop_between or i == 1):
            pops.append(C.pop(env))
            eps.append(env.pop_episode_stats())
    if not export:
        eps.append(env.pop_episode_stats())
    return SimpleNamespace(bufs=bufs, terms=np.array(terms) if terms else None, state=env.get_state(), pops=pops, eps=eps,
                           done=np.concatenate([b[5] for b in bufs]), faults=env.pop_fault_stats(), reruns=env.pop_rerun_count(),
                           queued=env.last_rollout_queued(), env=env)


def _same_outputs(a, b):
    for ra, rb in zip(a.bufs, b.bufs):
        for x, y in zip(ra, rb):
            np.testing.assert_array_equal(x, y)
    for x, y in zip(a.state, b.state):
        np.testing.assert_array_equal(x, y)


def _check_modes(env_name, N, monkeypatch, prepare=None, modes=("steps", "resident"), want_queue=False, want_reruns=False):
    runs = {}
    for mode in modes:
        off = _run(env_name, N, mode, False, monkeypatch, prepare)
        on = _run(env_name, N, mode, True, monkeypatch, prepare)
        split = _run(env_name, N, mode, True, monkeypatch, prepare, pop_between=True)
        print(f"--- {env_name} N={N} mode={mode}")
        _same_outputs(off, on)                                   # 1. bitwise neutrality (outputs and state)
        _same_outputs(off, split)
        assert off.faults == on.faults == (0, 0), (off.faults, on.faults)      # contact_overflow == 0 and diverged == 0
        assert (on.done != 0).any(axis=0).all(), "every env must end an episode"
        C.check_counts(on.pops[0], on.done, on.eps[0][2])        # 2. counts, exact
        assert on.eps[0][2] == off.eps[0][2]
        C.check_same_up_to_order(on.pops[0][0].sum(), on.eps[0][0], "sum of term sums vs ret_sum")      # 4.
        C.check_zero(C.pop(on.env))                              # 6. a second pop returns zeros ...
        C.check_counts(split.pops[0], split.done[:T1], split.eps[0][2])
        C.check_counts(split.pops[1], split.done[T1:], split.eps[1][2])
        C.check_same_up_to_order(split.pops[0][0] + split.pops[1][0], on.pops[0][0], "pop between the rollouts vs one pop")      # ... partial sums survive
        if want_queue and mode == "resident":
            assert on.queued and off.queued, "the job queue did not run"
        if want_reruns:
            assert on.reruns > 0 and on.reruns == off.reruns, (on.reruns, off.reruns)
        runs[mode] = on
    st = runs.get("steps")
    if st is not None:                                           # 3. against the host recomputation over the float32 read-backs
        assert st.terms.shape[:2] == st.done.shape
        host_sum, host_abs, _ = C.host_term_sums(st.terms, st.done)
        for mode, r in runs.items():
            np.testing.assert_array_equal(r.done, st.done)
            C.check_against_host(r.pops[0], host_sum, host_abs)
    if len(runs) == 2:                                           # 5. resident == launch per step up to the order of the atomics
        C.check_same_up_to_order(runs["resident"].pops[0][0], runs["steps"].pops[0][0], "resident vs launch per step")
        assert runs["resident"].pops[0][1:] == runs["steps"].pops[0][1:]
    return runs


@pytest.mark.parametrize("env_name", ["jvrc_walk", "h1", "h1_walk"])
def test_term_stats_two_envs_per_wave_tasks(env_name, monkeypatch):
    _check_modes(env_name, 97, monkeypatch)      # odd batch: the last wavefront holds one env


def test_term_stats_jvrc_step_through_the_job_queue(monkeypatch):
    monkeypatch.setenv("LHW_ROLLOUT_SLOTS", "48")      # fewer wave slots than envs: the resident waves drain the job queue
    monkeypatch.setenv("LHW_ROLLOUT_CHUNK", "5")
    _check_modes("jvrc_step", 131, monkeypatch, want_queue=True)


def test_term_stats_cartpole(monkeypatch):
    _check_modes("cartpole", 97, monkeypatch, modes=("steps",))      # (the lane-per-env stepper has no resident rollout)


def test_term_stats_count_an_in_wave_rerun_once(monkeypatch):
    """envs lying on the floor / tangled (the poses of tests/test_jvrc_gpu.py, as tests/test_rollout_resident_gpu.py places them): more
    than 8 contacts, so the two-envs-per-wave step hands them to the one-env-per-wave layout -- a second launch, or the same wavefront
    in the resident rollout.  The repeated control step must enter the statistics once."""
    poses = ([0.0, 0.0, 0.2571, -0.7309, -0.1371, 0.232, 0.627, -0.9859, -0.3243, -0.4729, 0.119, 0.609, 0.1118, -1.4146, 0.1458, 0.4932, 2.1903, 0.42, -0.5225],
             [0.0, 0.0, 0.1223, -0.4502, 0.0287, 0.3794, 0.8078, -1.2999, -0.2333, 0.4393, 0.4916, 0.2839, -0.8672, -1.533, 0.0192, -0.4235, 2.2823, -0.1645, -1.051],
             [0.0, 0.0, 0.142, -0.7055, -0.3568, 0.5444, 0.2804, 0.2372, -0.0299, -0.0106, 1.5965, -0.2912, -0.7387, -0.6059, -0.272, 0.0915, 0.445, -0.3003, 0.7158])

    def prepare(algo):
        env, ro = algo.env, algo.rollout
        ro.obs[ro.T].copy_(env.reset())      # (collect() continues from the last observation of the previous rollout)
        ro.started = True
        q, v = env.get_state()
        for i, pose in zip((0, 5, 15), poses):
            q[i] = pose
            q[i, 3:7] /= np.linalg.norm(q[i, 3:7])
            v[i] = 0
        env.set_state(q, v)
        env.pop_rerun_count()
        env.pop_episode_stats()
        if algo.term_stats_enabled:
            env.enable_term_stats(True)      # (re-arming zeroes the sums: the statistics start with the prepared state)

    runs = _check_modes("jvrc_walk", 16, monkeypatch, prepare=prepare, want_reruns=True)
    assert ((runs["steps"].done & 1) != 0).any(), "no env terminated"


def test_term_stats_against_the_oracle_reward_dictionaries():
    """The oracle env's float64 reward dictionary of every control step, summed per episode, against the device sums.  Tolerance: the
    per-step reward-term tolerance of tests/test_jvrc_gpu.py::test_action_tape_resynchronised (2e-6) times the number of steps summed."""
    from learninghumanoidwalking_amd.envs.jvrc_walk import JvrcWalkSpec
    from oracle.env_jvrc_walk import OracleJvrcWalkEnv
    N, T, L = 4, 24, 8
    spec = JvrcWalkSpec()
    env = spec.make_batched(N, seed=21, device=0, max_traj_len=L)
    orc = [OracleJvrcWalkEnv(spec, seed=21, env_id=i, max_traj_len=L) for i in range(N)]
    env.enable_term_stats(True)
    env.reset()
    for o in orc:
        o.reset()
    tape = (np.random.default_rng(7).normal(size=(T, N, 12)) * 0.4).astype(np.float32)
    run = np.zeros((N, 10))
    want, steps, counts = np.zeros(10), 0, [0, 0]
    length = np.zeros(N, int)
    for t in range(T):
        _, _, done, _ = env.step(torch.from_numpy(tape[t]).cuda())
        res = [o.step_auto(tape[t, i]) for i, o in enumerate(orc)]
        flags = np.array([r[2] for r in res], dtype=np.uint8)
        np.testing.assert_array_equal(done.cpu().numpy(), flags, err_msg=f"flags t={t}")
        for i, (r, o) in enumerate(zip(res, orc)):
            run[i] += [r[4][k] for k in o.TERMS]
            length[i] += 1
            if flags[i]:
                want += run[i]
                steps += length[i]
                counts[0 if flags[i] & 1 else 1] += 1
                run[i], length[i] = 0, 0
    stats = env.pop_term_stats()
    assert env.pop_fault_stats() == (0, 0)
    assert (stats["terminated"], stats["truncated"]) == tuple(counts) and stats["episodes"] == sum(counts) >= N * (T // L)
    got = np.array(list(stats["terms"].values())) * stats["episodes"]
    print("oracle leg: max |device - oracle|", np.abs(got - want).max(), "tol", 2e-6 * steps)
    assert list(stats["terms"]) == orc[0].TERMS
    np.testing.assert_allclose(got, want, rtol=0, atol=2e-6 * steps)
