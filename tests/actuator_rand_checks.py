"""Shared checks of the actuator randomisation (lhw_env_set_actuator_randomization / lhw_env_get_actuator_randomization /
lhw_env_get_bemf_damping, include/lhw.h: PD-gain noise and back-EMF damping of the reference's RobotBase, robots/robot_base.py:5-62) for
tests/test_actuator_rand.py (SIMT emulator) and tests/test_actuator_rand_gpu.py (the product BatchedEnv).  The float64 reference is
tests/actuator_rand_oracle.py; the backends and runners are those of tests/task_shaping_checks.py.

N = 3 envs throughout: one wavefront of the two-envs-per-wave kernels holds two envs, the next holds one."""
import ctypes

import numpy as np

from learninghumanoidwalking_amd import _lib
from tests import actuator_rand_oracle as O
from tests.task_shaping_checks import ERR_ARG, ERR_UNSUPPORTED, _np, _same, _same_state, spec_of

N = 3
DEFAULTS = dict(pdrand_k=0.0, sim_bemf=False, bemf_range=(5.0, 40.0), bemf_interval=10)
ENVS = ("jvrc_walk", "h1", "h1_walk", "jvrc_step")
# the tolerances of tests/test_emu_stepper.py::test_emulated_jvrc_perturbation
QPOS_ATOL, QVEL_ATOL, OBS_RTOL, OBS_ATOL, REW_ATOL = 1e-11, 1e-9, 1e-5, 2e-5, 2e-6
TAU_D_RTOL = 1e-14      # lo + (hi - lo) * u: the kernel may contract it into one FMA, nothing more
ACT_SCALE = {"jvrc_walk": 0.2, "h1": 0.08}


def step(env, act):
    """one control step of float32 actions [N][A] -> (obs, rew, done, rew_terms) host copies"""
    import torch
    obs, rew, done, _ = env.step(torch.from_numpy(np.ascontiguousarray(act, np.float32)).to(env.device))
    return _np(obs), _np(rew), _np(done), _np(env.rew_terms)


def reset(env, mask=None):
    import torch
    m = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask, np.uint8)).to(env.device)
    return _np(env.reset(m))


def tape(spec, name, T, seed=4):
    return (np.random.default_rng(seed).normal(size=(T, N, spec.act_dim)) * ACT_SCALE[name]).astype(np.float32)


def raw_set(env, pdrand_k=0.0, sim_bemf=0, bemf_interval=10, bemf_lo=5.0, bemf_hi=40.0):
    """the raw setter and its return code (values BatchedEnv would pass on unchanged, but whose refusal must not raise here)"""
    a = _lib.LhwActuatorRand(pdrand_k, sim_bemf, bemf_interval, bemf_lo, bemf_hi)
    return env._L.lhw_env_set_actuator_randomization(env._h, ctypes.byref(a))


# ---------------------------------------------------------------------------------------------------------------- 1 defaults, neutrality
def check_defaults_and_neutrality(backend, T=3):
    """a fresh env reports {0, 0, 10, 5, 40}; setting exactly that changes no bit of any output, resident and launch per step"""
    for name in ("jvrc_walk", "h1"):
        spec = spec_of(name)
        for mode in ("resident", "steps"):
            runs = []
            for touch in (False, True):
                env = backend.make(spec, N, seed=3, max_traj_len=2)
                assert env.actuator_randomization == DEFAULTS, env.actuator_randomization
                assert not env.bemf_damping().any() and env.bemf_damping().shape == (N, spec.act_dim)
                if touch:
                    env.set_actuator_randomization(**DEFAULTS)
                    assert env.actuator_randomization == DEFAULTS
                reset(env)
                b, terms = backend.runner(env, T, mode).collect()
                runs.append((env, b, terms))
            _same(runs[0][1], runs[1][1])
            _same_state(runs[0][0], runs[1][0])
            if terms is not None:
                np.testing.assert_array_equal(runs[0][2], runs[1][2])
            assert (runs[0][1]["done"] == 2).any(), "an auto-reset must be inside"
            for env, _, _ in runs:
                assert not env.bemf_damping().any()
                env.close()


# ---------------------------------------------------------------------------------------------------------------- 2, 3 oracle parity
def _parity(backend, name, seed, T, settings, twin_default=False, after_step=None):
    """T control steps of an action tape on a device env under `settings` against the oracle under the same; both sides (and the
    default twin) are put on the device's state after every step.  Returns the largest |qvel| difference of the default twin."""
    spec = spec_of(name)
    env = backend.make(spec, N, seed=seed)
    env.set_actuator_randomization(**settings)
    twin = backend.make(spec, N, seed=seed) if twin_default else None
    orc = [O.ORACLES[name](spec, seed=seed, env_id=i).configure(**settings) for i in range(N)]
    obs = reset(env)
    if twin is not None:
        reset(twin)
    ref = np.array([o.reset() for o in orc])
    np.testing.assert_allclose(obs, ref, rtol=OBS_RTOL, atol=OBS_ATOL)
    acts = tape(spec, name, T)
    twin_gap = 0.0
    for t in range(T):
        o_dev, rew, done, terms = step(env, acts[t])
        res = [o.step(acts[t, i]) for i, o in enumerate(orc)]
        q, v = env.get_state()
        oq, ov = np.array([o.sim.qpos.copy() for o in orc]), np.array([o.sim.qvel.copy() for o in orc])
        want_terms = np.array([[r[3][k] for k in o.TERMS] for r, o in zip(res, orc)])
        print(f"{name} t={t}: |dqpos| {np.abs(q - oq).max():.3e} |dqvel| {np.abs(v - ov).max():.3e} |dobs| {np.abs(o_dev - np.array([r[0] for r in res])).max():.3e} "
              f"|drew| {np.abs(rew - np.array([r[1] for r in res])).max():.3e} |dterms| {np.abs(terms - want_terms).max():.3e}  max |qvel| {np.abs(ov).max():.2f}")
        np.testing.assert_array_equal(done != 0, np.array([r[2] for r in res]), err_msg=f"flags t={t}")
        assert not done.any(), "the tape must keep every env inside its episode"
        np.testing.assert_allclose(q, oq, rtol=0, atol=QPOS_ATOL, err_msg=f"qpos t={t}")
        np.testing.assert_allclose(v, ov, rtol=0, atol=QVEL_ATOL, err_msg=f"qvel t={t}")
        np.testing.assert_allclose(o_dev, np.array([r[0] for r in res]), rtol=OBS_RTOL, atol=OBS_ATOL, err_msg=f"obs t={t}")
        np.testing.assert_allclose(rew, np.array([r[1] for r in res]), rtol=0, atol=REW_ATOL, err_msg=f"rew t={t}")
        np.testing.assert_allclose(terms, want_terms, rtol=0, atol=REW_ATOL, err_msg=f"terms t={t}")
        if after_step is not None:
            after_step(t, env, orc)
        if twin is not None:
            step(twin, acts[t])
            twin_gap = max(twin_gap, np.abs(twin.get_state()[1] - ov).max())
            twin.set_state(q, v)
        env.set_state(q, v)
        for i, o in enumerate(orc):
            o.set_state(q[i], v[i])
    assert env.pop_fault_stats() == (0, 0)
    env.close()
    if twin is not None:
        twin.close()
    return twin_gap


def check_pdrand_parity(backend, name, T=4):
    gap = _parity(backend, name, seed=17, T=T, settings=dict(pdrand_k=0.2), twin_default=True)
    print(name, "default env against the oracle with pdrand_k = 0.2: max |dqvel|", gap)
    assert gap > 1e-6, "the check would pass with the drawn gains ignored"


def bemf_seed(T):
    """the first seed for which some env fires by control step 3 and some env never fires in the T steps (interval 10)"""
    for seed in range(1, 1000):
        first = [next((t for t in range(T) if O.bemf_fires(seed, i, t)), None) for i in range(N)]
        if any(f is not None and f < 3 for f in first) and any(f is None for f in first):
            return seed, first
    raise AssertionError("no seed found")


def check_bemf_parity(backend, name, T=6):
    seed, first = bemf_seed(T)
    print(name, "seed", seed, "first firing step per env", first)
    assert any(f is not None and f < 3 for f in first) and any(f is None for f in first)      # (before the device runs)
    seen = []

    def tau_d(t, env, orc):
        got, want = env.bemf_damping(), np.array([o.tau_d for o in orc])
        np.testing.assert_allclose(got, want, rtol=TAU_D_RTOL, atol=0, err_msg=f"tau_d t={t}")
        seen.append(got)

    _parity(backend, name, seed=seed, T=T, settings=dict(sim_bemf=True), after_step=tau_d)
    for i, f in enumerate(first):
        for t in range(T):
            fired = f is not None and t >= f
            assert seen[t][i].all() == fired and seen[t][i].any() == fired, (i, t, seen[t][i])
            if fired:
                assert (seen[t][i] >= 5.0).all() and (seen[t][i] <= 40.0).all()


def check_bemf_survives_resets(backend, name):
    """tau_d across an auto-reset (max_traj_len = 3), across reset(mask), and zeroed by the call that turns sim_bemf off"""
    spec = spec_of(name)
    env = backend.make(spec, N, seed=5, max_traj_len=3)
    env.set_actuator_randomization(sim_bemf=True, bemf_interval=1)      # (every control step redraws)
    reset(env)
    acts = tape(spec, name, 3)
    step(env, acts[0])
    step(env, acts[1])
    before = env.bemf_damping()
    assert before.all() and len(np.unique(before)) == before.size
    env.set_actuator_randomization(sim_bemf=True, bemf_interval=2**30)      # (never again; a setter that keeps sim_bemf on keeps tau_d)
    np.testing.assert_array_equal(env.bemf_damping(), before)
    _, _, done, _ = step(env, acts[2])
    assert (done == 2).all(), done      # every env was truncated and reset itself inside this control step
    np.testing.assert_array_equal(env.bemf_damping(), before)
    reset(env, mask=[1, 0, 1])
    np.testing.assert_array_equal(env.bemf_damping(), before)
    reset(env)
    np.testing.assert_array_equal(env.bemf_damping(), before)
    env.set_actuator_randomization(pdrand_k=0.1, sim_bemf=True)      # (another knob changes: kept)
    np.testing.assert_array_equal(env.bemf_damping(), before)
    env.set_actuator_randomization(pdrand_k=0.1, sim_bemf=False)
    assert not env.bemf_damping().any()
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 4, 5 resident == steps
BOTH = dict(pdrand_k=0.2, sim_bemf=True, bemf_interval=2)


def check_resident_equals_steps(backend, name, stats, T=4):
    """both knobs: the resident rollout (plain, or with the term statistics) is bitwise the launch-per-step loop, tau_d included"""
    spec = spec_of(name)
    out = {}
    for mode in ("resident", "steps", "off"):
        env = backend.make(spec, N, seed=11, max_traj_len=3)
        if mode != "off":
            env.set_actuator_randomization(**BOTH)
        if stats:
            env.enable_term_stats()
        reset(env)
        b, _ = backend.runner(env, T, "steps" if mode == "off" else mode).collect()
        out[mode] = (env, b, env.bemf_damping(), env.pop_term_sums() if stats else None)
    (er, br, tr, sr), (es, bs, ts, ss), (eo, bo, to, _) = out["resident"], out["steps"], out["off"]
    _same(br, bs)
    _same_state(er, es)
    np.testing.assert_array_equal(tr, ts)
    assert tr.any() and not to.any(), "the back-EMF draw must have fired somewhere (interval 2, 3 envs, 4 steps)"
    assert not np.array_equal(bs["rew"], bo["rew"]), "the randomisation must show in the rewards"
    assert (bs["done"] == 2).any(), "an auto-reset must be inside"
    if stats:
        np.testing.assert_array_equal(sr[0], ss[0])
        assert sr[1:] == ss[1:] and sr[1] + sr[2] > 0
    for e in (er, es, eo):
        e.close()


def check_setter_between_rollouts(backend, T=3):
    """two resident rollouts with the setter between them == launch per step with the call at the same step"""
    spec = spec_of("jvrc_walk")
    out = {}
    for mode in ("resident", "steps", "never"):
        env = backend.make(spec, N, seed=7, max_traj_len=4)
        reset(env)
        r = backend.runner(env, T, "resident" if mode == "never" else mode)
        b1, _ = r.collect()
        if mode != "never":
            env.set_actuator_randomization(pdrand_k=0.3, sim_bemf=True, bemf_interval=1)
        b2, _ = r.collect()
        out[mode] = (env, b1, b2)
    _same(out["resident"][1], out["steps"][1])
    _same(out["resident"][1], out["never"][1])
    _same(out["resident"][2], out["steps"][2])
    _same_state(out["resident"][0], out["steps"][0])
    np.testing.assert_array_equal(out["resident"][0].bemf_damping(), out["steps"][0].bemf_damping())
    assert out["resident"][0].bemf_damping().all()
    assert not np.array_equal(out["never"][2]["rew"], out["resident"][2]["rew"]), "the call must take effect with the next control step"
    for e, _, _ in out.values():
        e.close()


# ---------------------------------------------------------------------------------------------------------------- 6 what declines
def check_clocks_exclude(backend):
    """the kernels with the diagnostic clocks carry no actuator randomisation: whichever is armed first refuses the other"""
    spec = spec_of("jvrc_walk")
    env = backend.make(spec, N, seed=1)
    env.set_actuator_randomization(pdrand_k=0.1)
    for call in (env.wave_cycles, env.phase_cycles):
        try:
            call()
            raise AssertionError("a clock was armed beside the actuator randomisation")
        except _lib.LhwError as e:
            assert e.code == ERR_UNSUPPORTED and "actuator randomisation" in str(e), e
    env.set_actuator_randomization()      # off again: the clock can be armed ...
    env.wave_cycles()
    for kw in (dict(pdrand_k=0.1), dict(sim_bemf=1)):      # ... and then refuses the setter, which changes nothing
        assert raw_set(env, **kw) == ERR_UNSUPPORTED and b"clock" in env._L.lhw_last_error()
        assert env.actuator_randomization == DEFAULTS
    assert raw_set(env) == 0      # (setting "off" is no conflict)
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 7 refusals
def check_refusals(backend):
    from learninghumanoidwalking_amd.envs import CartpoleSpec
    nan, inf = float("nan"), float("inf")
    env = backend.make(spec_of("jvrc_walk"), N, seed=1)
    env.set_actuator_randomization(pdrand_k=0.25, sim_bemf=True, bemf_range=(6.0, 30.0), bemf_interval=1)
    reset(env)
    step(env, np.zeros((N, 12), np.float32))
    state, tau_d = env.actuator_randomization, env.bemf_damping()
    assert tau_d.all()
    cases = [(dict(pdrand_k=-0.1), b"pdrand_k"), (dict(pdrand_k=1.0), b"pdrand_k"), (dict(pdrand_k=nan), b"pdrand_k"), (dict(pdrand_k=inf), b"pdrand_k"),
             (dict(bemf_interval=0), b"bemf_interval"), (dict(bemf_interval=-3), b"bemf_interval"),
             (dict(bemf_lo=-1.0), b"bemf_lo"), (dict(bemf_lo=nan), b"bemf_lo"), (dict(bemf_lo=inf, bemf_hi=inf), b"bemf_lo"),
             (dict(bemf_lo=41.0), b"bemf_hi"), (dict(bemf_hi=nan), b"bemf_hi"), (dict(bemf_hi=inf), b"bemf_hi")]
    for kw, word in cases:
        rc = raw_set(env, **kw)
        msg = env._L.lhw_last_error()
        assert rc == ERR_ARG and word in msg, (kw, rc, msg)
        assert env.actuator_randomization == state
        np.testing.assert_array_equal(env.bemf_damping(), tau_d)
    env.close()
    env = backend.make(CartpoleSpec(), 2, seed=1)
    a = _lib.LhwActuatorRand()
    out = np.zeros((2, 1))
    for rc in (raw_set(env, pdrand_k=0.1), env._L.lhw_env_get_actuator_randomization(env._h, ctypes.byref(a)),
               env._L.lhw_env_get_bemf_damping(env._h, out.ctypes.data)):
        assert rc == ERR_UNSUPPORTED and b"humanoid" in env._L.lhw_last_error()
    env.close()
