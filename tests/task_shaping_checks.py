"""Shared checks of the task shaping (lhw_env_set_task_shaping / lhw_env_get_task_shaping, include/lhw.h: the reward-term weights and
termination bounds of the fused humanoid tasks as run-time settings) for tests/test_task_shaping.py (SIMT emulator) and
tests/test_task_shaping_gpu.py (the product BatchedEnv).  The reference keeps these numbers as literals of tasks/walking_task.py,
stepping_task.py and standing_task.py; the reference for OTHER values is the shipped plug-in of the same task (task_hook.Vector*Task,
which tests/test_task_hook*.py and tests/test_task_inputs.py pin to the reference's tasks/rewards.py), constructed with the same
weights and bounds and evaluated in float64 on the task-input record the same control step exported.

A Backend makes envs -- the product's BatchedEnv on a GPU or on the emulated library -- and `runners`: T control steps of a random actor,
as ONE resident rollout or launch per step.  Everything else goes through BatchedEnv's own methods; the raw C ABI only where a call is
made that the class refuses to make (check_errors)."""
import ctypes
import os

import numpy as np

from learninghumanoidwalking_amd import _lib

REW_ATOL = 1e-6       # float32 rew_terms / rew against the float64 reference: the figure of tests/test_task_inputs.py.  Holds while every
                      # weight lies in [0, 1] and the weights sum to <= 2: a raw term is at most 1 (exp of a non-positive number; the clock
                      # terms tan(pi/4 * [-1, 1])), so |w * term| <= 1, float32 rounding <= 2^-24 = 6e-8 per term and 10 of them in the sum
ERR_ARG, ERR_UNSUPPORTED = -1, -4
ENVS = ("jvrc_walk", "h1", "h1_walk", "jvrc_step")


# ---------------------------------------------------------------------------------------------------------------- the env's calls
def get_shaping(env):
    """(weights [n_terms], limits [2]) float64, read back from the library"""
    w, lim = env.task_shaping()
    assert tuple(w) == _lib.REWARD_TERMS[env.task]
    return np.array(list(w.values())), np.array(lim)


def set_shaping_rc(env, weights=None, limits=None, n_weights=None, n_limits=None):
    """the raw setter and its return code (check_errors: counts that do not match the arrays, values the library must refuse)"""
    w = None if weights is None else np.ascontiguousarray(weights, np.float64)
    lim = None if limits is None else np.ascontiguousarray(limits, np.float64)
    return env._L.lhw_env_set_task_shaping(env._h, None if w is None else w.ctypes.data, (0 if w is None else w.size) if n_weights is None else n_weights,
                                           None if lim is None else lim.ctypes.data, (0 if lim is None else lim.size) if n_limits is None else n_limits)


def set_shaping(env, weights=None, limits=None):
    env.set_task_shaping(reward_weights=weights, termination=limits)


def shaped_weights(n):
    """pairwise different (a swapped index shows), each in [0, 1], sum 1.1 for ten terms (REW_ATOL)"""
    return 0.02 * (np.arange(n) + 1.0)


def _np(x):
    return x.detach().cpu().numpy().copy() if hasattr(x, "detach") else np.array(x, copy=True)


def step(env, act):
    """one control step of float32 actions [N][A] -> (rew [N], done [N], rew_terms [N][K]) host copies"""
    import torch
    _, rew, done, _ = env.step(torch.from_numpy(np.ascontiguousarray(act, np.float32)).to(env.device))
    return _np(rew), _np(done), _np(env.rew_terms)


def arm_records(env):
    env.enable_task_inputs()
    if env.task == _lib.TASK_JVRC_STEP:
        env.enable_step_task_inputs()


def record_rows(fields, table, dim):
    """the [N][dim] float64 record whose named fields (BatchedEnv.get_task_inputs / get_step_task_inputs) are `fields`"""
    n = len(next(iter(fields.values())))
    rec = np.zeros((n, dim))
    for k, v in fields.items():
        v = np.asarray(v).reshape(n, -1)
        rec[:, table[k][0]:table[k][0] + v.shape[1]] = v
    return rec


def records(env):
    """the task-input record(s) of the last control step as a task_hook.TaskInputs of float64 CPU tensors"""
    import torch
    from learninghumanoidwalking_amd.task_hook import TaskInputs
    rec = record_rows(env.get_task_inputs(), _lib.TASK_INPUT_FIELDS, _lib.TASK_INPUT_DIM)
    srec = None
    if env.task == _lib.TASK_JVRC_STEP:
        srec = torch.from_numpy(record_rows(env.get_step_task_inputs(), _lib.STEP_TASK_INPUT_FIELDS, _lib.STEP_TASK_INPUT_DIM))
    return TaskInputs(torch.from_numpy(rec), env.nq, env.nv, env.act_dim, srec)


def reference_task(spec, weights, limits):
    """the shipped plug-in of the spec's task with these weights [K] and bounds (lo, hi), on the CPU"""
    from learninghumanoidwalking_amd.task_hook import VectorStandingTask, VectorSteppingTask, VectorWalkingTask
    names = _lib.REWARD_TERMS[spec.task_code]
    w = dict(zip(names, (float(x) for x in weights)))
    if spec.task_code == _lib.TASK_JVRC_STEP:
        return VectorSteppingTask(spec, "cpu", weights=w, min_root_height=float(limits[0]))
    cls = VectorStandingTask if spec.task_code == _lib.TASK_H1_STAND else VectorWalkingTask
    return cls(spec, "cpu", weights=w, height_limits=(float(limits[0]), float(limits[1])))


def height(spec, ti):
    """what the termination bounds apply to: root z, or (stepping) root z above the lower foot site"""
    import torch
    if spec.task_code == _lib.TASK_JVRC_STEP:
        return (ti.root_xpos[:, 2] - torch.minimum(ti.lsite_xpos[:, 2], ti.rsite_xpos[:, 2])).numpy()
    return ti.qpos[:, 2].numpy().copy()


def spec_of(name):
    from learninghumanoidwalking_amd.envs import ENVIRONMENTS
    return ENVIRONMENTS[name]()


def tape(spec, N, T=8, seed=5):
    return (np.random.default_rng(seed).normal(size=(T, N, spec.act_dim)) * 0.3).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- backends
class EmuRunner:
    """T control steps of a random numpy actor on an emulated env (the helpers of tests/test_rollout_resident.py / test_term_stats.py)"""

    def __init__(self, env, T, mode):
        from tests import emu
        from tests.test_rollout_resident import NumpyActor
        self.env, self.T, self.mode = emu.numpy_face(env), T, mode
        self.pol = NumpyActor(env.obs_dim, env.act_dim, seed=5, scale=2.0)
        self.obs = np.zeros((env.n_envs, env.obs_dim), np.float32)

    def collect(self):
        """-> (buffers {obs act logp tob rew done}, rew_terms [T][N][K] (launch per step only))"""
        from tests.test_rollout_resident import _resident
        from tests.test_term_stats import _per_step_with_terms
        if self.mode == "resident":
            b, terms = _resident(self.env, self.pol, self.T, self.obs), None
        else:
            b, terms = _per_step_with_terms(self.env, self.pol, self.T, self.obs)
        self.pol.view.counter += self.T
        self.obs = b["obs"][self.T].copy()
        return b, terms


class GpuRunner:
    """T control steps of the product's Rollout (feed-forward actor with the reference's initial weights) on a BatchedEnv"""

    def __init__(self, env, T, mode):
        from learninghumanoidwalking_amd.ppo import Rollout
        from learninghumanoidwalking_amd.ppo_kernels import PpoKernels, reference_init
        k = PpoKernels(env.obs_dim, env.act_dim, hidden=256, max_rows=256)
        k.set_tensors(reference_init(env.obs_dim, env.act_dim, 256, 0.223, generator_seed=0))
        self.env, self.T, self.mode = env, T, mode
        self.ro = Rollout(env, k, T, seed=5)
        self.ro.obs[T].zero_()          # (collect() continues from the last observation of the previous rollout: start from zeros, like EmuRunner)
        self.ro.started = True

    def collect(self):
        env, ro, terms = self.env, self.ro, []
        orig, before = env.step, os.environ.get("LHW_ROLLOUT_MODE")

        def stepped(*a, **k):
            r = orig(*a, **k)
            terms.append(_np(env.rew_terms))
            return r

        os.environ["LHW_ROLLOUT_MODE"] = self.mode
        if self.mode == "steps":
            env.step = stepped
        try:
            ro.collect()
        finally:
            if self.mode == "steps":
                del env.step
            if before is None:
                del os.environ["LHW_ROLLOUT_MODE"]
            else:
                os.environ["LHW_ROLLOUT_MODE"] = before
        assert ro.last_mode == self.mode, ro.last_mode
        b = dict(obs=_np(ro.obs), act=_np(ro.act), logp=_np(ro.logp), tob=_np(ro.tob_all), rew=_np(ro.rew), done=_np(ro.done))
        return b, (np.array(terms) if terms else None)


class Backend:
    """`runner` (EmuRunner / GpuRunner: they differ in the actor) and where its envs live: `device`, and for the emulator `library`, a
    function that returns the handle (so that importing a test file builds nothing)"""

    def __init__(self, runner, device, library=None):
        self.runner, self.device, self.library = runner, device, library

    def make(self, spec, N, seed, max_traj_len=0):
        where = {} if self.library is None else dict(library=self.library())
        return spec.make_batched(N, seed=seed, device=self.device, max_traj_len=max_traj_len, **where)


def _same(a, b):
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def _same_state(x, y):
    for a, b in zip(x.get_state(), y.get_state()):
        np.testing.assert_array_equal(a, b)


N1, T1, L1 = 5, 9, 4      # the set-up of tests/test_term_stats.py: an odd batch, every env truncates twice, envs 0 and 3 lie on the floor


LIFT = 0.04               # env 2 starts this far above the nominal root height: inside the reference's limits, above the tightened upper one


def tight(spec):
    """bounds that bite where the reference's do not: a lower one inside the 0.78 - 0.83 the root height of a standing, randomly actuated
    JVRC takes (check_limits prints it), an upper one between the nominal height and the lifted env 2"""
    return (0.80, float(spec.nominal_pose[2]) + LIFT / 2)


def _fallen_env(backend, stats=False):
    from tests.test_rollout_resident import _fallen_states
    spec = spec_of("jvrc_walk")
    env = backend.make(spec, N1, seed=3, max_traj_len=L1)
    env.reset()
    q, v = _fallen_states(spec, N1, seed=21)
    q[2, 2] += LIFT
    env.set_state(q, v)
    env.pop_rerun_count()
    if stats:
        from tests import term_stats_checks as C
        C.enable(env)
    return env


# ---------------------------------------------------------------------------------------------------------------- the checks
def check_defaults(backend):
    """check 1, second half: a fresh env reports the reference's numbers (and the Python tables say the same)"""
    for name in ENVS:
        spec = spec_of(name)
        env = backend.make(spec, 2, seed=1)
        w, lim = get_shaping(env)
        print(name, "weights", w, "limits", lim)
        np.testing.assert_array_equal(w, np.array(_lib.DEFAULT_REWARD_WEIGHTS[spec.task_code]))
        np.testing.assert_array_equal(lim, np.array(_lib.DEFAULT_TERMINATION[spec.task_code]))
        ref = reference_task(spec, w, lim)      # ... which are the shipped plug-in's, i.e. the reference's tasks/*_task.py
        assert [ref.w[k] for k in ref.TERMS] == list(w) and tuple(ref.TERMS) == _lib.REWARD_TERMS[spec.task_code]
        assert tuple(lim) == {"jvrc_walk": (0.6, 1.4), "h1_walk": (0.6, 1.4), "h1": (0.9, 1.4), "jvrc_step": (0.6, np.inf)}[name]
        env.close()


def check_neutrality(backend):
    """check 1: never touched == set to the getter's values == only weights / only limits set, bitwise, resident and launch per step"""
    for mode in ("resident", "steps"):
        runs = []
        for touch in ("never", "both", "weights" if mode == "resident" else "limits"):      # (the other half NULL)
            env = _fallen_env(backend)
            w, lim = get_shaping(env)
            if touch == "both":
                set_shaping(env, w, lim)
            elif touch == "weights":
                set_shaping(env, w, None)
            elif touch == "limits":
                set_shaping(env, None, lim)
            b, _ = backend.runner(env, T1, mode).collect()
            runs.append((env, b))
        for env, b in runs[1:]:
            _same(runs[0][1], b)
            _same_state(runs[0][0], env)
        done = runs[0][1]["done"]
        assert ((done & 1) != 0).any() and ((done & 2) != 0).any(axis=0).all(), "terminations and truncations must be inside"
        reruns = [env.pop_rerun_count() for env, _ in runs]
        assert reruns[0] > 0 and len(set(reruns)) == 1, reruns      # the W = 64 re-run of the fallen envs is inside
        for env, _ in runs:
            env.close()


def check_weights(backend, name):
    """check 2: rew_terms and rew under pairwise different weights against the float64 plug-in on the same step's record"""
    import torch
    spec = spec_of(name)
    N = 4
    env = backend.make(spec, N, seed=5)
    K = env.n_terms
    w = shaped_weights(K)
    set_shaping(env, w, None)
    got_w, lim = get_shaping(env)
    np.testing.assert_array_equal(got_w, w)
    ref = reference_task(spec, w, lim)
    arm_records(env)
    env.reset()
    acts = tape(spec, N)
    raw_max = np.zeros(K)
    for t in range(len(acts)):
        rew, _, terms = step(env, acts[t])
        want_rew, _ = ref.evaluate(records(env))
        want = torch.stack([ref.last_terms[k] for k in ref.TERMS], dim=1).numpy()
        err_t, err_r = np.abs(terms - want).max(), np.abs(rew - want_rew.numpy()).max()
        print(f"{name} t={t}: max |rew_terms - ref| {err_t:.3e}  max |rew - ref| {err_r:.3e}")
        np.testing.assert_allclose(terms, want, rtol=0, atol=REW_ATOL, err_msg=f"{name} rew_terms t={t}")
        np.testing.assert_allclose(rew, want_rew.numpy(), rtol=0, atol=REW_ATOL, err_msg=f"{name} rew t={t}")
        raw_max = np.maximum(raw_max, (terms / w).max(axis=0))
    print(name, "largest raw value of each term", raw_max)
    assert (raw_max > 1e-3).all(), f"a term never showed its weight: {raw_max}"
    # a weight of exactly 0 gives exactly 0.0f
    w0 = w.copy()
    w0[K // 2] = 0.0
    set_shaping(env, w0, None)
    _, _, terms = step(env, acts[0])
    assert (terms[:, K // 2] == 0.0).all() and not np.signbit(terms[:, K // 2]).any(), terms[:, K // 2]
    assert (terms[:, np.arange(K) != K // 2] != 0.0).any(axis=0).all()
    env.close()


def check_limits(backend, name):
    """check 3: termination flags under bounds set inside the range the height actually takes, exact against the rule on the record"""
    spec = spec_of(name)
    N = 4
    stepping = spec.task_code == _lib.TASK_JVRC_STEP
    acts = tape(spec, N)

    def run(limits, T=len(acts)):
        env = backend.make(spec, N, seed=5, max_traj_len=0)
        if limits is not None:
            set_shaping(env, None, limits)
        w, lim = get_shaping(env)
        ref = reference_task(spec, w, lim)
        arm_records(env)
        env.reset()
        zs, flags = [], []
        for t in range(T):
            _, done, _ = step(env, acts[t])
            ti = records(env)
            _, want = ref.evaluate(ti)
            np.testing.assert_array_equal((done & 1) != 0, want.numpy(), err_msg=f"{name} limits {lim} t={t}")
            zs.append(height(spec, ti))
            flags.append(done & 1)
        env.close()
        return np.array(zs), np.array(flags)

    z, flags = run(None)
    print(name, "height under the reference's limits: min", z.min(), "max", z.max())
    assert not flags.any(), "no env may terminate under the reference's limits on this tape"
    lo, hi = np.percentile(z, 30), (np.inf if stepping else np.percentile(z, 70))
    z2, flags2 = run((lo, hi))
    below, above = z2 < lo, z2 > hi
    print(name, "limits", (lo, hi), "env-steps below / above / inside", below.sum(), above.sum(), (~below & ~above).sum(), "terminated", flags2.sum())
    assert below.any() and (~below & ~above).any() and (stepping or above.any()), "the tape must meet every case of the rule"
    assert (flags2[below | above] == 1).all() and flags2.sum() >= (below | above).sum()
    # an infinite bound is switched off (run() holds every flag to the rule; with both off only a self collision could end an episode)
    for limits in ((-np.inf, hi), (lo, np.inf)):
        if limits != (lo, hi):
            run(limits, T=3)
    assert not run((-np.inf, np.inf), T=3)[1].any()


def check_resident_equals_steps(backend):
    """check 4: under other weights and a tightened lower bound the resident rollout is bitwise the launch-per-step loop, and the per-term
    statistics are the host's sums of rew_terms over the finished episodes"""
    from tests import term_stats_checks as C
    out = {}
    for mode in ("resident", "steps"):
        env = _fallen_env(backend, stats=True)
        set_shaping(env, shaped_weights(env.n_terms), tight(spec_of("jvrc_walk")))
        b, terms = backend.runner(env, T1, mode).collect()
        out[mode] = (env, b, terms, C.pop(env), env.pop_episode_stats())
    (er, br, _, pr, epr), (es, bs, terms, ps, eps) = out["resident"], out["steps"]
    _same(br, bs)
    _same_state(er, es)
    done = bs["done"]
    standing = [n for n in range(N1) if n not in (0, 3)]
    print("terminations per env", ((done & 1) != 0).sum(axis=0), "truncations per env", (done == 2).sum(axis=0))
    assert done[0, 2] & 1, "the tightened upper bound must end the lifted env's episode at once"
    assert not (done[0, [1, 4]] & 1).any()
    assert (done == 2).any(), "some episodes must still reach max_traj_len"
    C.check_counts(pr, done, epr[2])
    C.check_counts(ps, done, eps[2])
    host_sum, host_abs, _ = C.host_term_sums(terms, done)
    C.check_against_host(pr, host_sum, host_abs)
    C.check_against_host(ps, host_sum, host_abs)
    er.close(), es.close()


def check_setter_mid_run(backend):
    """check 5: two resident rollouts of T = 4 with a setter call between them == launch per step with the call at the same step"""
    T = 4
    out = {}
    for mode in ("resident", "steps"):
        env = _fallen_env(backend)
        r = backend.runner(env, T, mode)
        b1, _ = r.collect()
        set_shaping(env, shaped_weights(env.n_terms), tight(spec_of("jvrc_walk")))
        b2, _ = r.collect()
        out[mode] = (env, b1, b2)
    _same(out["resident"][1], out["steps"][1])
    _same(out["resident"][2], out["steps"][2])
    _same_state(out["resident"][0], out["steps"][0])
    # the call took effect: the same second rollout without it gives other rewards
    env = _fallen_env(backend)
    r = backend.runner(env, T, "resident")
    r.collect()
    b2, _ = r.collect()
    assert not np.array_equal(b2["rew"], out["resident"][2]["rew"])
    for e in (env, out["resident"][0], out["steps"][0]):
        e.close()


def check_errors(backend):
    """check 6: refused calls name their cause and change nothing"""
    from learninghumanoidwalking_amd.envs import CartpoleSpec
    for name in ("jvrc_walk", "jvrc_step"):
        spec = spec_of(name)
        env = backend.make(spec, 2, seed=1)
        K = env.n_terms
        w0, lim0 = get_shaping(env)
        w = shaped_weights(K)
        bad_w = w.copy()
        bad_w[1] = np.nan
        inf_w = w.copy()
        inf_w[0] = np.inf
        hi = np.inf if name == "jvrc_step" else 1.3
        cases = [(dict(weights=w, n_weights=K - 1), b"n_weights"), (dict(weights=w, n_weights=K + 1), b"n_weights"),
                 (dict(limits=(0.5, hi), n_limits=1), b"n_limits"), (dict(limits=(0.5, hi), n_limits=3), b"n_limits"),
                 (dict(weights=bad_w), b"finite"), (dict(weights=inf_w), b"finite"), (dict(limits=(np.nan, hi)), b"NaN"),
                 (dict(limits=(0.5, np.nan)), b"NaN"), (dict(limits=(0.7, 0.7)), b"below"), (dict(limits=(np.inf, np.inf)), b"below"),
                 (dict(weights=w, limits=(0.9, 0.5)), b"below")]
        if name == "jvrc_step":
            cases.append((dict(limits=(0.5, 1.4)), b"upper"))
        for kw, word in cases:
            rc = set_shaping_rc(env, **kw)
            msg = env._L.lhw_last_error()
            assert rc == ERR_ARG and word in msg, (name, kw, rc, msg)
            w1, lim1 = get_shaping(env)
            np.testing.assert_array_equal(w1, w0)      # (the refused call with good weights and bad limits changed neither half)
            np.testing.assert_array_equal(lim1, lim0)
        set_shaping(env, -w, (0.5, hi))      # negative weights are a penalty, not an error
        w1, lim1 = get_shaping(env)
        np.testing.assert_array_equal(w1, -w)
        np.testing.assert_array_equal(lim1, (0.5, hi))
        env.close()
    env = backend.make(CartpoleSpec(), 2, seed=1)
    assert set_shaping_rc(env, np.ones(4), None) == ERR_UNSUPPORTED
    w, lim = np.zeros(4), np.zeros(2)
    assert env._L.lhw_env_get_task_shaping(env._h, w.ctypes.data, lim.ctypes.data) == ERR_UNSUPPORTED
    env.close()
