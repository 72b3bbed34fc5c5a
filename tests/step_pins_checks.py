"""Shared checks of the stepping task's pinned walk modes and footstep plans (lhw_env_pin_step_plans / lhw_env_get_pinned_step_plans,
include/lhw.h; BatchedEnv.pin_step_plans / unpin_step_plans / pinned_step_plans) for tests/test_step_pins.py (SIMT emulator) and
tests/test_step_pins_gpu.py (the product BatchedEnv).  The reference draws the mode and the plan inside SteppingTask.reset
(tasks/stepping_task.py:261-334, 140-182); what a pinned env must do instead is stated by the oracle's stepping env with `_generate`
overridden (PinnedPlans below): a pin replaces the RESULT of the draw it names and nothing else.  The backends and runners are those of
tests/task_shaping_checks.py.

N = 3 envs throughout: env 0 carries an explicit plan, env 1 is free, env 2 is pinned to a mode."""
import ctypes

import numpy as np

from learninghumanoidwalking_amd import _lib
from oracle import rng
from oracle.env_jvrc_step import BACKWARD, CURVED, FORWARD, LATERAL, STANDING, OracleJvrcStepEnv
from tests.task_commands_checks import OBS_ATOL, OBS_RTOL, QPOS_ATOL, QVEL_ATOL, REW_ATOL, step
from tests.task_shaping_checks import ERR_ARG, ERR_UNSUPPORTED, _np, _same, _same_state, spec_of

N = 3
SEQ_ATOL = 1e-12      # the sequence against the oracle's: metres, a handful of roundings, an FMA's difference at most
MODES = _lib.STEP_COMMAND_MODES
assert [MODES.index(m) for m in ("curved", "standing", "backward", "lateral", "forward")] == [CURVED, STANDING, BACKWARD, LATERAL, FORWARD]
# check 3, env 0: six steps at FORWARD's own spacing (0.3 m ahead, 0.15 m to either side) that climb AND turn -- the reference generates
# stairs (z) only on straight plans and turns (theta) only on flat ones
PLAN0 = np.array([[0.0, 0.1, 0.0, 0.0], [0.3, -0.15, 0.0, 0.0], [0.6, 0.15, 0.0, 0.05], [0.9, -0.15, 0.03, 0.1], [1.2, 0.15, 0.06, 0.1],
                  [1.5, -0.15, 0.06, 0.15]])
HEIGHT2 = 0.07        # check 3, env 2: FORWARD with this rise per step at iteration 0, where the schedule gives 0


# ---------------------------------------------------------------------------------------------------------------- the oracle
class PinnedPlans:
    """Mixin in front of OracleJvrcStepEnv with the pin rule of include/lhw.h.  `pin`: None (free) or a dict(mode=, choice=-1,
    height=nan, steps=None).  _task_reset calls _generate right behind the mode draw and reads self.mode afterwards (the floor), so the
    override takes the pinned mode there; every draw is still made (`dr`), a pinned value stands for the RESULT of its draw."""
    pin = None

    def _generate(self, dr):
        p = self.pin
        if p is None:
            return super()._generate(dr)
        self.mode = int(p["mode"])
        if p.get("steps") is not None:
            return [np.array(s, dtype=float) for s in p["steps"]]
        choice, height = p.get("choice", -1), p.get("height", np.nan)
        if choice >= 0:
            dr = dict(dr, choice=choice, plan=choice)
        if self.mode != FORWARD or np.isnan(height):
            return super()._generate(dr)
        # FORWARD with a pinned rise: generate_step_sequence (stepping_task.py:140-182) with step_height = height
        u, gap = dr["first_u"], 0.15
        neg = self.phase == 0.5 * self.period
        seq, y = [np.array([0.0, -1 * u if neg else 1 * u, 0.0, 0.0])], -gap if neg else gap
        x, z = 0.0, 0.0
        for i in range(1, 20 - 1):
            x += 0.3
            y *= -1
            if i > dr["cflat"]:
                z += height
            seq.append(np.array([x, y, z, 0.0]))
        seq.append(np.array([x + 0.3, -y, z, 0.0]))
        return seq


class PinnedJvrcStep(PinnedPlans, OracleJvrcStepEnv):
    pass


def oracles(seed, pins=None, max_traj_len=0, iteration=0):
    spec = spec_of("jvrc_step")
    out = []
    for i in range(N):
        o = PinnedJvrcStep(spec, seed=seed, env_id=i, max_traj_len=max_traj_len)
        o.pin, o.iteration_count = (pins or {}).get(i), iteration
        out.append(o)
    return out


def drawn(o, c):
    """what env `o` (an oracle, its iteration set) draws at reset number c, as the fields of a pin: (mode, choice, height, steps) with
    `steps` the generated sequence [n][4] -- recomputed from oracle.rng, no physics involved"""
    dr = o._draws(c)
    u = dr["mode_u"]
    mode = CURVED if u < 0.15 else (STANDING if u < 0.2 else (BACKWARD if u < 0.4 else (LATERAL if u < 0.7 else FORWARD)))
    keep = o.mode, o.phase, o.pin
    o.mode, o.phase, o.pin = mode, (int(o.period / 2) if dr["phase_half"] else 0), None
    steps = np.array(o._generate(dr))
    o.mode, o.phase, o.pin = keep
    choice, height = -1, np.nan
    if mode == CURVED:
        choice = int(dr["plan"])
    elif mode == LATERAL:
        choice = int(dr["choice"])
    elif mode == FORWARD:
        hh = np.clip((o.iteration_count - 3000) / 8000, 0, 1) * 0.1
        height = -hh if dr["choice"] == 0 else hh
    return mode, choice, height, steps


def _mode_of(seed, env, c):
    u = rng.u01(seed, env, rng.STREAM_RESET, c, 1)
    return CURVED if u < 0.15 else (STANDING if u < 0.2 else (BACKWARD if u < 0.4 else (LATERAL if u < 0.7 else FORWARD)))


def _cover_seed(resets=2):
    """the first seed whose three envs draw FORWARD, LATERAL and CURVED (in any order) at their first reset and modes that differ from
    those at the next -- found on the CPU, as tests/task_commands_checks.py::_forward_seed finds its seed"""
    for seed in range(1, 5000):
        first = [_mode_of(seed, i, 0) for i in range(N)]
        if set(first) == {FORWARD, LATERAL, CURVED} and any(_mode_of(seed, i, 1) != first[i] for i in range(N)):
            return seed
    raise AssertionError("no seed found")


# ---------------------------------------------------------------------------------------------------------------- the env's calls
def reset(env):
    return _np(env.reset())


def tape(T, seed=5, scale=0.1):
    return (np.random.default_rng(seed).normal(size=(T, N, 12)) * scale).astype(np.float32)


def snapshot(env):
    """everything a control step leaves behind that the host can read: state and the stepping task's record"""
    return tuple(env.get_state()) + tuple(env.debug_step_record())


WHAT = ("obs", "rew", "done", "terms", "qpos", "qvel", "sequence", "floor", "istate")


def run(env, acts, before_step=None):
    """the tape, launch per step -> per step (obs, rew, done, terms, qpos, qvel, sequence, floor, istate)"""
    out = []
    for t in range(len(acts)):
        if before_step is not None:
            before_step(t, out)
        out.append(step(env, acts[t]) + snapshot(env))
    return out


def same_runs(a, b, envs=range(N), what="run"):
    assert len(a) == len(b)
    for t, (x, y) in enumerate(zip(a, b)):
        for u, v, name in zip(x, y, WHAT):
            np.testing.assert_array_equal(u[list(envs)], v[list(envs)], err_msg=f"{what}: {name} t={t}")


def raw_pin(env, first, pins):
    pins = np.ascontiguousarray(pins, dtype=_lib.STEP_PIN_DTYPE)
    return env._L.lhw_env_pin_step_plans(env._h, int(first), len(pins), pins.ctypes.data)


def pin_record(mode=-1, choice=-1, nseq=0, reserved=0, height=np.nan, steps=None):
    r = np.zeros(1, dtype=_lib.STEP_PIN_DTYPE)
    r["mode"], r["choice"], r["nseq"], r["reserved"], r["height"] = mode, choice, nseq, reserved, height
    if steps is not None:
        r["steps"][0, :len(steps)] = steps
    return r


def no_pin(env):
    p = env.pinned_step_plans()
    return bool((p["mode"] == -1).all()) and not any(p[k].any() for k in ("choice", "nseq", "reserved", "height", "steps"))


def pin_check3(env):
    env.pin_step_plans("forward", steps=PLAN0, envs=0)
    env.pin_step_plans("forward", height=HEIGHT2, envs=[2])


# ---------------------------------------------------------------------------------------------------------------- 1 neutrality
def check_neutrality(backend, seed=4, T=6):
    """pins on envs 0 and 2 beside a twin without any pin call: env 1 bitwise the twin's; after unpin_step_plans() every reset draws
    what the twin's draws"""
    spec = spec_of("jvrc_step")
    acts = tape(T)
    pinned, twin = backend.make(spec, N, seed=seed, max_traj_len=4), backend.make(spec, N, seed=seed, max_traj_len=4)
    assert no_pin(pinned) and no_pin(twin)      # (before the first pin call the getter reports a batch of free envs)
    pin_check3(pinned)
    o0, o1 = reset(pinned), reset(twin)
    np.testing.assert_array_equal(o0[1], o1[1])
    a, b = run(pinned, acts), run(twin, acts)
    same_runs(a, b, envs=[1], what="free env beside pinned envs")
    done = np.array([x[2] for x in a])
    assert (done != 0).any(), "an auto-reset must be inside"
    np.testing.assert_array_equal(done, np.array([x[2] for x in b]))      # (every env has made the same resets on both sides)
    assert not np.array_equal(a[-1][6][[0, 2]], b[-1][6][[0, 2]]), "the pinned envs must differ from their free twins"
    pinned.unpin_step_plans()
    assert no_pin(pinned)
    # The reset behind the unpin draws what the twin draws.  Its three settle steps stand on the terrain of the episode before
    # (base_humanoid_env.py:247-276) -- the pinned one here, the drawn one there -- so the feet the plan is laid out from, and with them
    # the state, differ in their last digits for envs 0 and 2 from then on: what a reset DRAWS is compared exactly (mode, floor, the
    # target state machine, every step's z), env 1 stays bit for bit
    o0, o1 = reset(pinned), reset(twin)
    np.testing.assert_array_equal(o0[1], o1[1])
    (sa, fa, ia), (sb, fb, ib) = pinned.debug_step_record(), twin.debug_step_record()
    np.testing.assert_array_equal(fa, fb)
    np.testing.assert_array_equal(ia, ib)
    np.testing.assert_array_equal(sa[:, :, 2], sb[:, :, 2])
    np.testing.assert_array_equal(sa[1], sb[1])
    for e in (pinned, twin):
        e.enable_task_inputs()
    a, b = run(pinned, acts), run(twin, acts)
    same_runs(a, b, envs=[1], what="free env behind the unpin")
    np.testing.assert_array_equal(pinned.get_task_inputs()["mode"], twin.get_task_inputs()["mode"])
    np.testing.assert_array_equal(a[-1][8][:, 4], b[-1][8][:, 4])      # (the plans the auto-reset inside this run laid out: the same draws again)
    pinned.close(), twin.close()


# ---------------------------------------------------------------------------------------------------------------- 2 the identity
def check_pinning_what_was_drawn_is_the_identity(backend, T=6, L=4, iteration=7000):
    """a free run against twins pinned to exactly what each env draws -- (mode, choice, height) alone, then with the generated sequence
    as an explicit plan as well -- bitwise over T steps with an auto-reset inside; the pins of the next reset go in one step ahead"""
    spec = spec_of("jvrc_step")
    seed = _cover_seed()
    acts = tape(T)
    orc = oracles(seed, iteration=iteration)
    hh = np.clip((iteration - 3000) / 8000, 0, 1) * 0.1
    assert hh == 0.05

    free = backend.make(spec, N, seed=seed, max_traj_len=L)
    free.set_iteration(iteration)
    free.enable_task_inputs()
    obs_free = reset(free)
    first = [drawn(o, 0) for o in orc]
    assert {d[0] for d in first} == {FORWARD, LATERAL, CURVED}
    seq, floor, ist = free.debug_step_record()
    np.testing.assert_array_equal(floor, [-2.0 if d[0] == FORWARD else 0.0 for d in first])      # (the recomputed draws are the env's)
    np.testing.assert_array_equal(ist[:, 4], [len(d[3]) for d in first])
    for d in first:
        if d[0] == FORWARD:
            assert abs(d[2]) == hh and set(np.round(np.diff(d[3][:, 2]), 12)) == {0.0, round(d[2], 12)}
    ref = run(free, acts)
    np.testing.assert_array_equal(free.get_task_inputs()["mode"], [_mode_of(seed, i, 1) for i in range(N)])
    done = np.array([x[2] for x in ref])
    assert (done[L - 1] != 0).all() and not done[:L - 1].any(), "every env truncates at step L and none ends before"

    for explicit in (False, True):
        twin = backend.make(spec, N, seed=seed, max_traj_len=L)
        twin.set_iteration(iteration)
        twin.enable_task_inputs()

        def pin(c):
            for i, o in enumerate(orc):
                mode, choice, height, steps = drawn(o, c)
                twin.pin_step_plans(mode, choice=choice, height=height, steps=steps if explicit else None, envs=i)

        pin(0)
        got = twin.pinned_step_plans()
        assert list(got["mode"]) == [d[0] for d in first] and list(got["nseq"]) == [len(d[3]) if explicit else 0 for d in first]
        np.testing.assert_array_equal(reset(twin), obs_free)
        pin(1)      # acts at the auto-reset inside step L; a pin never acts inside an episode
        same_runs(run(twin, acts, before_step=lambda t, out: pin(2) if t == L else None), ref, what=f"pinned to the draws (explicit plan: {explicit})")
        twin.close()
    free.close()


# ---------------------------------------------------------------------------------------------------------------- 3 the oracle
def check_against_oracle(backend, seed=7, T=6):
    """env 0: an explicit 6-step plan that climbs and turns; env 1: free; env 2: FORWARD rising 0.07 per step at iteration 0"""
    spec = spec_of("jvrc_step")
    env = backend.make(spec, N, seed=seed)
    pin_check3(env)
    got = env.pinned_step_plans()
    assert list(got["mode"]) == [FORWARD, -1, FORWARD] and list(got["nseq"]) == [6, 0, 0] and got["height"][2] == HEIGHT2
    np.testing.assert_array_equal(got["steps"][0, :6], PLAN0)
    orc = oracles(seed, pins={0: dict(mode=FORWARD, steps=PLAN0), 2: dict(mode=FORWARD, height=HEIGHT2)})
    env.enable_task_inputs()

    def compare(t, obs, want_obs):
        seq, floor, ist = env.debug_step_record()
        q, v = env.get_state()
        oq, ov = np.array([o.sim.qpos.copy() for o in orc]), np.array([o.sim.qvel.copy() for o in orc])
        want_seq = np.array([o.sequence for o in orc])
        print(f"t={t}: |dseq| {np.abs(seq[:, :, :4] - want_seq).max():.3e} |dqpos| {np.abs(q - oq).max():.3e} |dqvel| {np.abs(v - ov).max():.3e} "
              f"|dobs| {np.abs(obs - want_obs).max():.3e} t1 {ist[:, 0]} t2 {ist[:, 1]} nseq {ist[:, 4]} floor {floor}")
        np.testing.assert_allclose(seq[:, :, :4], want_seq, rtol=0, atol=SEQ_ATOL, err_msg=f"sequence t={t}")
        np.testing.assert_array_equal(floor, [-2.0 if o.mode == FORWARD else 0.0 for o in orc], err_msg=f"floor t={t}")
        np.testing.assert_array_equal(ist[:, [0, 1, 4]], [[o.t1, o.t2, o.nseq] for o in orc], err_msg=f"t1 t2 nseq t={t}")
        np.testing.assert_allclose(q, oq, rtol=0, atol=QPOS_ATOL, err_msg=f"qpos t={t}")
        np.testing.assert_allclose(v, ov, rtol=0, atol=QVEL_ATOL, err_msg=f"qvel t={t}")
        np.testing.assert_allclose(obs, want_obs, rtol=OBS_RTOL, atol=OBS_ATOL, err_msg=f"obs t={t}")

    obs, want = reset(env), np.array([o.reset() for o in orc])
    compare("reset", obs, want)
    assert [o.mode for o in orc][::2] == [FORWARD, FORWARD] and [o.nseq for o in orc][::2] == [6, 20]
    dz = np.diff(orc[2].sequence[:, 2])
    assert set(np.round(dz, 12)) == {0.0, HEIGHT2} and orc[0].sequence[3, 2] == 0.03 and orc[0].sequence[5, 3] != orc[0].sequence[0, 3]
    acts = tape(T)
    for t in range(T):
        o_dev, rew, done, terms = step(env, acts[t])
        res = [o.step(acts[t, i]) for i, o in enumerate(orc)]
        compare(t, o_dev, np.array([r[0] for r in res]))
        want_rew = np.array([r[1] for r in res])
        print(f"t={t}: |drew| {np.abs(rew - want_rew).max():.3e} flags {done}")
        np.testing.assert_allclose(rew, want_rew, rtol=0, atol=REW_ATOL, err_msg=f"rew t={t}")
        np.testing.assert_array_equal(done != 0, [r[2] for r in res], err_msg=f"done t={t}")
        np.testing.assert_array_equal(env.get_task_inputs()["mode"], [o.mode for o in orc], err_msg=f"LHW_TIN_MODE t={t}")
    assert env.pop_fault_stats() == (0, 0)
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 4 resident == steps
def _resident_with_records(backend, env, T, obs0):
    """ONE resident launch of a random feed-forward actor with both task-input records -> numpy dict (obs act logp tob rew done tin stin)"""
    import torch
    from learninghumanoidwalking_amd.batched_env import BatchedEnv
    n, D, A, dev = env.n_envs, env.obs_dim, env.act_dim, env.device
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)      # noqa: E731
    b = dict(obs=z(T + 1, n, D), act=z(T, n, A), logp=z(T, n), tob=z(T, n, D), rew=z(T, n), done=z(T, n, dt=torch.uint8))
    b["obs"][0] = torch.as_tensor(obs0).to(dev)
    tin = torch.full((T, n, _lib.TASK_INPUT_DIM), float("nan"), dtype=torch.float64, device=dev)
    stin = torch.full((T, n, _lib.STEP_TASK_INPUT_DIM), float("nan"), dtype=torch.float64, device=dev)
    if backend.library is not None:      # the emulated library reads a policy of host arrays
        from tests.test_rollout_resident import NumpyActor
        pol = NumpyActor(D, A, seed=5, scale=2.0)
        assert BatchedEnv.rollout(env, pol.view, T, *b.values(), task_inputs=tin, step_task_inputs=stin)
    else:
        from learninghumanoidwalking_amd.ppo_kernels import PpoKernels, reference_init
        k = PpoKernels(D, A, hidden=256, max_rows=256)
        k.set_tensors(reference_init(D, A, 256, 0.223, generator_seed=0))
        k.begin_rollout()
        try:
            assert BatchedEnv.rollout(env, k.rollout_policy(seed=1, counter=0, deterministic=False), T, *b.values(), task_inputs=tin, step_task_inputs=stin)
        finally:
            k.end_rollout()
        torch.cuda.synchronize()
    return dict({k: _np(v) for k, v in b.items()}, tin=_np(tin), stin=_np(stin))


def expected_targets(seq, stin_fields):
    """target1 / target2 of a stepping record against the sequence rows its t1 / t2 name"""
    for i in range(len(seq)):
        np.testing.assert_array_equal(stin_fields["target1"][i], seq[i, int(stin_fields["t1"][i]), :4])
        np.testing.assert_array_equal(stin_fields["target2"][i], seq[i, int(stin_fields["t2"][i]), :4])


def check_resident_equals_steps(backend, seed=7, T=8, L=4):
    """one resident launch across two auto-resets against the launch-per-step loop on the same actions: every buffer, both records and
    the state bitwise; the pinned envs carry their pinned mode and plan behind the in-launch resets too"""
    spec = spec_of("jvrc_step")
    res, per = backend.make(spec, N, seed=seed, max_traj_len=L), backend.make(spec, N, seed=seed, max_traj_len=L)
    for e in (res, per):
        pin_check3(e)
    o0, o1 = reset(res), reset(per)
    np.testing.assert_array_equal(o0, o1)
    r = _resident_with_records(backend, res, T, o0)
    per.enable_task_inputs()
    per.enable_step_task_inputs()
    m0 = _lib.TASK_INPUT_FIELDS["mode"][0]
    for t in range(T):
        obs, rew, done, _ = step(per, r["act"][t])
        for got, name in ((obs, "obs"), (rew, "rew"), (done, "done")):
            np.testing.assert_array_equal(got, r[name][t + 1 if name == "obs" else t], err_msg=f"{name} t={t}")
        srec = np.concatenate([v.reshape(N, -1) for v in per.get_step_task_inputs().values()], axis=1)
        np.testing.assert_array_equal(srec, r["stin"][t, :, :srec.shape[1]], err_msg=f"stepping record t={t}")
        np.testing.assert_array_equal(per.get_task_inputs()["mode"], r["tin"][t, :, m0], err_msg=f"mode t={t}")
        assert list(r["tin"][t, [0, 2], m0]) == [FORWARD, FORWARD]      # (pinned, whichever episode the step belongs to)
        if not done.any():      # (the record of a step that ends an episode holds that episode's targets, the env already the next plan)
            fields = _lib.split_step_task_inputs(r["stin"][t])
            expected_targets(per.debug_step_record()[0], fields)
            assert list(fields["nseq"][[0, 2]]) == [6, 20] and fields["target1"][0, 2] in PLAN0[:, 2]
    _same_state(res, per)
    for a, b in zip(res.debug_step_record(), per.debug_step_record()):
        np.testing.assert_array_equal(a, b)
    assert (r["done"][L - 1] != 0).all() and (r["done"][T - 1] != 0).all(), "two auto-resets must be inside the launch"
    # behind the in-launch resets the pinned envs hold their plans again, transformed at THAT reset: z as given, theta relative to the first step's
    seq, floor, ist = res.debug_step_record()
    assert list(ist[[0, 2], 4]) == [6, 20] and list(floor[[0, 2]]) == [-2.0, -2.0]
    np.testing.assert_array_equal(seq[0, :6, 2], PLAN0[:, 2])
    np.testing.assert_allclose(seq[0, :6, 3] - seq[0, 0, 3], PLAN0[:, 3], rtol=0, atol=SEQ_ATOL)
    assert set(np.round(np.diff(seq[2, :, 2]), 12)) == {0.0, HEIGHT2}
    res.close(), per.close()


# ---------------------------------------------------------------------------------------------------------------- 5 refusals, getter
def check_refusals_and_getter(backend):
    from learninghumanoidwalking_amd.envs import CartpoleSpec
    nan, inf = float("nan"), float("inf")
    spec = spec_of("jvrc_step")
    env = backend.make(spec, N, seed=1)
    nplans = len(spec.plans)
    pin_check3(env)
    env.pin_step_plans("lateral", choice=1, envs=1)
    state = env.pinned_step_plans().tobytes()
    bad_steps = PLAN0.copy()
    bad_steps[4, 2] = inf
    nan_steps = PLAN0.copy()
    nan_steps[0, 3] = nan
    cases = [((0, pin_record(mode=5)), b"mode"), ((0, pin_record(mode=-2)), b"mode"), ((0, pin_record(mode=CURVED, choice=nplans)), b"choice"),
             ((0, pin_record(mode=CURVED, choice=-2)), b"choice"), ((0, pin_record(mode=LATERAL, choice=2)), b"choice"),
             ((0, pin_record(mode=FORWARD, choice=0)), b"choice"), ((0, pin_record(mode=STANDING, choice=1)), b"choice"),
             ((0, pin_record(mode=BACKWARD, choice=0)), b"choice"), ((0, pin_record(mode=FORWARD, nseq=1, steps=PLAN0)), b"nseq"),
             ((0, pin_record(mode=FORWARD, nseq=21, steps=PLAN0)), b"nseq"), ((0, pin_record(mode=FORWARD, nseq=-1)), b"nseq"),
             ((0, pin_record(mode=FORWARD, nseq=6, steps=bad_steps)), b"steps"), ((0, pin_record(mode=CURVED, nseq=6, steps=nan_steps)), b"steps"),
             ((0, pin_record(mode=FORWARD, height=inf)), b"height"), ((0, pin_record(mode=FORWARD, height=-inf)), b"height"),
             ((0, pin_record(mode=FORWARD, reserved=1)), b"reserved"), ((0, pin_record(mode=-1, reserved=7)), b"reserved"),
             ((-1, pin_record(mode=FORWARD)), b"batch"), ((N, pin_record(mode=FORWARD)), b"batch"),
             ((N - 1, np.concatenate([pin_record(mode=FORWARD)] * 2)), b"batch"),
             # a good row in front of a bad one: nothing of the call is applied
             ((0, np.concatenate([pin_record(mode=STANDING), pin_record(mode=9)])), b"mode")]
    for (first, pins), word in cases:
        rc = raw_pin(env, first, pins)
        msg = env._L.lhw_last_error()
        assert rc == ERR_ARG and word in msg, (first, pins[["mode", "choice", "nseq", "reserved", "height"]], rc, msg)
        assert env.pinned_step_plans().tobytes() == state
    assert raw_pin(env, N, pin_record()[:0]) == 0      # (an empty range at the end of the batch is a range of the batch)
    assert env.pinned_step_plans().tobytes() == state
    # the edges are values: the last plan, 2 and 20 steps, a NaN height (the schedule's), a finite one on a mode that does not read it
    long_plan = np.tile(PLAN0[:4], (5, 1))
    for rec in (pin_record(mode=CURVED, choice=nplans - 1), pin_record(mode=FORWARD, nseq=2, steps=PLAN0), pin_record(mode=STANDING, nseq=20, steps=long_plan),
                pin_record(mode=FORWARD, height=nan), pin_record(mode=LATERAL, choice=0, height=0.5)):
        assert raw_pin(env, 1, rec) == 0, env._L.lhw_last_error()
    # getter -> setter changes no bit (a NaN height and a free env among them)
    env.unpin_step_plans(envs=2)
    before = env.pinned_step_plans()
    assert before["mode"][2] == -1 and not before["steps"][2].any() and before["height"][2] == 0 and np.isnan(before["height"][0])
    assert raw_pin(env, 0, before) == 0, env._L.lhw_last_error()
    assert env.pinned_step_plans().tobytes() == before.tobytes()
    # steps behind nseq are not part of the pin: they read back as zeros
    rec = pin_record(mode=FORWARD, nseq=3, steps=PLAN0)
    assert raw_pin(env, 0, rec) == 0
    got = env.pinned_step_plans()[0]
    np.testing.assert_array_equal(got["steps"][:3], PLAN0[:3])
    assert not got["steps"][3:].any()
    # an [n][3] plan of x, y, theta gets z = 0
    env.pin_step_plans("curved", steps=PLAN0[:, [0, 1, 3]], envs=0)
    got = env.pinned_step_plans()[0]
    np.testing.assert_array_equal(got["steps"][:6], np.insert(PLAN0[:, [0, 1, 3]], 2, 0.0, axis=1))
    assert got["mode"] == CURVED and got["nseq"] == 6
    # the walking tasks' pin still refuses the stepping task
    modes, refs = np.array([2], np.int32), np.zeros((1, 3))
    assert env._L.lhw_env_pin_commands(env._h, 0, 1, modes.ctypes.data, refs.ctypes.data) == ERR_UNSUPPORTED
    env.close()
    out = np.zeros(2, dtype=_lib.STEP_PIN_DTYPE)
    for other in (spec_of("jvrc_walk"), spec_of("h1"), CartpoleSpec()):
        env = backend.make(other, 2, seed=1)
        for rc in (raw_pin(env, 0, pin_record(mode=FORWARD)), env._L.lhw_env_get_pinned_step_plans(env._h, out.ctypes.data)):
            assert rc == ERR_UNSUPPORTED and b"jvrc_step" in env._L.lhw_last_error(), (rc, env._L.lhw_last_error())
        env.close()
    assert ctypes.sizeof(_lib.LhwStepPin) == 4 * 4 + 8 + 20 * 4 * 8 == _lib.STEP_PIN_DTYPE.itemsize
