"""The Gaussian policy head -- the exploration noise and the stored log-density of every rollout row -- against its float64
restatement, oracle/policy_head.py (reference semantics: torch.distributions.Normal, rl/policies/actor.py:160-188):

  a. the restatement's noise is N(0,1), independent across envs, control steps and action components (properties of the keying design);
  b. csrc/lhw_policy.h compiled for the host agrees with it pointwise on > 1e5 keys, the edges of the key space included;
  c. every call site on the SIMT emulator (the two reference policy launches and the three resident rollouts) agrees with it pointwise:
     the key each one forms -- seed, env_id_base + env, counter + t, slots 2a / 2a + 1 -- and the std column it reads.

Bounds: tests/policy_head_checks.py.  GPU twin: tests/test_policy_head_gpu.py."""
import ctypes
import math
import subprocess

import numpy as np
import pytest

from oracle import policy_head as ph
from oracle import rng
from tests.policy_head_checks import CASES, COUNTER0, ENV_BASE, SEED, check_head, head_case, rollout_keys

EDGE_KEYS = [  # (seed, env, counter): the corners of the key space
    (0, 0, 0), (0, 2**32 - 1, 0), (0, 0, 2**32 - 1), (2**63, 0, 0), (2**64 - 1, 2**32 - 1, 2**32 - 1), (2**63 + 5, 2**32 - 2, 2**31),
    (3, 2**31, 2**31 - 1), (2**63 - 1, 2**32 - 1, 1)]


def _random_keys(n, rs):
    seed = rs.integers(0, 2**64, size=n, dtype=np.uint64)
    env = rs.integers(0, 2**32, size=n, dtype=np.uint64)
    counter = rs.integers(0, 2**32, size=n, dtype=np.uint64)
    for i, (s, e, c) in enumerate(EDGE_KEYS):
        seed[i], env[i], counter[i] = s, e, c
    return seed, env, counter


# ------------------------------------------------------------------------------------------------------------------ the restatement itself

def test_vectorised_bits_are_the_integer_restatement():
    """oracle/policy_head.py's numpy-uint64 bits / u01 == oracle/rng.py's Python-integer ones on 400 keys: random 64 / 32-bit keys of every
    stream, the edge keys (env 2**32 - 1: env + 1 wraps to 0 as in lhw_rng.h's uint32_t; counter 2**32 - 1; seeds >= 2**63)."""
    rs = np.random.default_rng(0)
    n = 400
    seed, env, counter = _random_keys(n, rs)
    stream = rs.integers(1, 4, size=n, dtype=np.uint64)
    slot = rs.integers(0, 64, size=n, dtype=np.uint64)
    slot[:4] = (0, 2**32 - 1, 2**16, 63)
    got = ph.bits(seed, env, stream, counter, slot)
    gotu = ph.u01(seed, env, stream, counter, slot)
    for i in range(n):
        k = tuple(int(v[i]) for v in (seed, env, stream, counter, slot))
        assert int(got[i]) == rng.bits(*k), k
        assert gotu[i] == rng.u01(*k), k
    assert ((0 <= gotu) & (gotu < 1)).all()
    # the wrap: env 2**32 - 1 is the key of "env -1", and scalars broadcast like arrays
    assert rng.bits(7, 2**32 - 1, 3, 5, 1) == rng.splitmix64(rng.splitmix64(7) ^ (3 << 56) ^ (5 << 16) ^ 1)
    assert int(ph.bits(7, 2**32 - 1, 3, 5, 1)) == rng.bits(7, 2**32 - 1, 3, 5, 1)
    assert rng.bits(7, 2**32 - 1, 3, 5, 1) != rng.bits(7, 2**32 - 2, 3, 5, 1)


def test_restatement_formulas_on_scalars():
    """normal64 / sample64 / log_density64 spelled out with the math module on Python-integer uniforms"""
    for seed, env, counter in EDGE_KEYS + [(3, 17, 9)]:
        for a in (0, 1, 11, 31):
            u1, u2 = rng.u01(seed, env, rng.STREAM_POLICY, counter, 2 * a), rng.u01(seed, env, rng.STREAM_POLICY, counter, 2 * a + 1)
            z = math.sqrt(-2.0 * math.log(1.0 - u1)) * math.cos(6.283185307179586 * u2)
            got = float(ph.normal64(seed, env, counter, a))
            assert abs(got - z) <= 4e-16 * max(1.0, abs(z)), (seed, env, counter, a)
    mu, sd = np.array([0.5, -1.0, 2.0]), np.array([0.25, 1.5, 0.1])
    x = ph.sample64(mu, sd, 3, 17, 9)
    np.testing.assert_array_equal(x, mu + sd * ph.normal64(3, 17, 9, np.arange(3)))
    np.testing.assert_array_equal(ph.sample64(mu, sd, 3, 17, 9, deterministic=True), mu)
    want = sum(-0.5 * ((xi - m) / s) ** 2 - math.log(s) - 0.5 * math.log(2 * math.pi) for xi, m, s in zip(x, mu, sd))
    assert abs(float(ph.log_density64(x, mu, sd)) - want) < 1e-14
    # batched keys: [T][N] rows
    env, counter = rollout_keys(2, 3)
    xb = ph.sample64(np.broadcast_to(mu, (2, 3, 3)), sd, 3, np.broadcast_to(env, (2, 3)), np.broadcast_to(counter, (2, 3)))
    assert xb[1, 2, 1] == mu[1] + sd[1] * float(ph.normal64(3, ENV_BASE + 2, COUNTER0 + 1, 1))
    assert ph.noise_block(3, ENV_BASE, 3, COUNTER0, 2, 3)[1, 2, 1] == float(ph.normal64(3, ENV_BASE + 2, COUNTER0 + 1, 1))


# ------------------------------------------------------------------------------------------------------------------ a. statistical battery

BLOCKS = {  # name: (seed, env base, envs, counter base, steps, actions)
    "seed3": (3, 0, 1024, 0, 32, 12),
    "seed123-env4096-counter1000": (123, 4096, 1024, 1000, 32, 12),
    "seed0-64steps-32actions": (0, 0, 256, 0, 64, 32),
    "seed2^63+5-counter2^31": (2**63 + 5, 0, 1024, 2**31, 32, 10),
}
_PHI = np.vectorize(lambda v: 0.5 * (1.0 + math.erf(v / math.sqrt(2.0))))


def battery(z):
    """every statistic of z [T][N][A] in units of its standard error under iid N(0,1) (KS: D sqrt(n)), and max |z|"""
    n = z.size
    out = {"mean": z.mean() * math.sqrt(n), "m2": ((z ** 2).mean() - 1.0) / math.sqrt(2.0 / n),
           "m3": (z ** 3).mean() / math.sqrt(15.0 / n), "m4": ((z ** 4).mean() - 3.0) / math.sqrt(96.0 / n)}
    for name, axis in (("lag_counter", 0), ("lag_env", 1), ("lag_action", 2)):
        a, b = np.moveaxis(z, axis, 0)[:-1], np.moveaxis(z, axis, 0)[1:]
        out[name] = (a * b).mean() * math.sqrt(a.size)      # (a product of two independent N(0,1) has variance 1)
    s = np.sort(z, axis=None)
    F = _PHI(s)
    i = np.arange(1, n + 1)
    out["ks"] = max((i / n - F).max(), (F - (i - 1) / n).max()) * math.sqrt(n)
    out["max_abs"] = np.abs(z).max()
    return {k: float(v) for k, v in out.items()}


@pytest.mark.parametrize("block", list(BLOCKS))
def test_noise_is_standard_normal_and_uncorrelated_across_env_step_and_action(block):
    """Mean, second, third and fourth raw moment (standard errors 1/sqrt n, sqrt(2/n), sqrt(15/n), sqrt(96/n) under N(0,1)) and the lag-1
    correlation along the env, the counter and the action axis (1/sqrt n) within 5 standard errors; Kolmogorov-Smirnov against Phi with
    D sqrt n < 2.0 (asymptotic tail 2 exp(-2 * 2.0^2) = 6.7e-4).  Measured, in standard errors (KS: D sqrt n):

      block                         n       mean    m2     m3     m4    lag_counter  lag_env  lag_action   KS    max |z|
      seed3                        393216  -1.21  -1.43  -0.60  -0.86     +0.51      -1.48     -1.41     0.96    4.62
      seed123-env4096-counter1000  393216  -0.89  -1.28  -0.54  -1.70     -0.64      -2.22     -0.45     0.88    4.85
      seed0-64steps-32actions      524288  -0.82  -0.25  -0.36  +0.54     -0.44      +1.81     -1.50     0.83    4.84
      seed2^63+5-counter2^31       327680  -0.04  -0.81  +0.65  -1.24     +1.55      +0.36     +0.39     0.56    5.03
    """
    seed, env_base, n_envs, counter_base, T, A = BLOCKS[block]
    z = ph.noise_block(seed, env_base, n_envs, counter_base, T, A)
    assert z.shape == (T, n_envs, A) and np.isfinite(z).all()
    st = battery(z)
    print(block, z.size, " ".join(f"{k}={v:+.2f}" for k, v in st.items()))
    for k in ("mean", "m2", "m3", "m4", "lag_counter", "lag_env", "lag_action"):
        assert abs(st[k]) < 5.0, (block, k, st[k])
    assert st["ks"] < 2.0, (block, st["ks"])
    assert st["max_abs"] <= 8.6      # sqrt(-2 log 2^-53): the largest a 53-bit uniform can give


def test_battery_notices_what_it_is_for():
    """the battery on noise with keying mistakes: one slot for both uniforms, a key that ignores the env, a counter that does not advance"""
    seed, A, N, T = 3, 12, 256, 32
    a = np.arange(A, dtype=np.uint64)[None, None, :]
    n = np.arange(N, dtype=np.uint64)[None, :, None]
    t = np.arange(T, dtype=np.uint64)[:, None, None]
    u = lambda slot, env=n, ctr=t: ph.u01(seed, env, rng.STREAM_POLICY, ctr, slot) + 0.0 * (n + t + a)
    bm = lambda u1, u2: np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(ph.TWO_PI * u2)
    same_slot = battery(bm(u(2 * a), u(2 * a)))
    assert same_slot["ks"] > 2.0
    no_env = battery(bm(u(2 * a, env=0 * n), u(2 * a + 1, env=0 * n)))
    assert abs(no_env["lag_env"]) > 5.0
    no_counter = battery(bm(u(2 * a, ctr=0 * t), u(2 * a + 1, ctr=0 * t)))
    assert abs(no_counter["lag_counter"]) > 5.0


# ------------------------------------------------------------------------------------------------------------------ b. the header on the host

SHIM = r"""
#include <math.h>
#include "lhw_policy.h"
void head_rows(long n, int A, const float* mu, const float* sd, const uint64_t* seed, const uint32_t* env, const uint32_t* counter, int det, float* act, float* logp) {
  for (long i = 0; i < n; i++) {
    float lp = 0.f, term;
    for (int a = 0; a < A; a++) { act[i * A + a] = lhw_policy_sample(mu[i * A + a], sd[a], seed[i], env[i], counter[i], a, det, &term); lp += term; }
    logp[i] = lp;
  }
}
void rng_bits(long n, const uint64_t* seed, const uint32_t* env, const uint32_t* stream, const uint32_t* counter, const uint32_t* slot, uint64_t* out) {
  for (long i = 0; i < n; i++) out[i] = lhw_rng_bits(seed[i], env[i], stream[i], counter[i], slot[i]);
}
"""


@pytest.fixture(scope="module")
def host_head(tmp_path_factory):
    from tests import emu
    d = tmp_path_factory.mktemp("policy_head_shim")
    src, so = d / "shim.c", d / "libshim.so"
    src.write_text(SHIM)
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", emu._CSRC, str(src), "-o", str(so), "-lm"])
    return ctypes.CDLL(str(so))


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def test_header_rng_on_the_host_is_the_oracle_rng_at_the_key_edges(host_head):
    """lhw_rng_bits compiled by gcc == oracle/rng.py == oracle/policy_head.py on the edge keys and 5000 random ones"""
    rs = np.random.default_rng(1)
    n = 5000
    seed, env, counter = _random_keys(n, rs)
    stream = rs.integers(1, 4, size=n, dtype=np.uint64)
    slot = rs.integers(0, 2**32, size=n, dtype=np.uint64)
    out = np.zeros(n, np.uint64)
    u32 = [np.ascontiguousarray(v, np.uint32) for v in (env, stream, counter, slot)]
    host_head.rng_bits(ctypes.c_long(n), _p(seed), _p(u32[0]), _p(u32[1]), _p(u32[2]), _p(u32[3]), _p(out))
    np.testing.assert_array_equal(out, ph.bits(seed, env, stream, counter, slot))
    for i in range(len(EDGE_KEYS) + 50):
        assert int(out[i]) == rng.bits(int(seed[i]), int(env[i]), int(stream[i]), int(counter[i]), int(slot[i]))


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("A", [12, 32])
def test_header_on_the_host_against_the_restatement(host_head, case, A):
    """lhw_policy_sample over 10000 rows x A actions (1.2e5 / 3.2e5 keys per case; the edge keys in the first rows), sampled and
    deterministic.  Largest error / bound (gcc, glibc): action 0.996 (a float32 rounding of z that all but reaches half an ulp), log-density 0.134."""
    rs = np.random.default_rng(A)
    n = 10000
    seed, env, counter = _random_keys(n, rs)
    b3, sd, exact = head_case(case, A)
    mu = np.ascontiguousarray(np.broadcast_to(b3, (n, A)))
    if not exact:
        mu = (mu + rs.normal(size=(n, A)).astype(np.float32)).astype(np.float32)
    e32, c32 = np.ascontiguousarray(env, np.uint32), np.ascontiguousarray(counter, np.uint32)
    for det in (0, 1):
        act, logp = np.zeros((n, A), np.float32), np.zeros(n, np.float32)
        host_head.head_rows(ctypes.c_long(n), A, _p(mu), _p(sd), _p(seed), _p(e32), _p(c32), det, _p(act), _p(logp))
        r = check_head(act, logp, mu, sd, seed, env, counter, exact_fma=exact, deterministic=bool(det), what=f"host {case} A={A} det={det}")
        print(f"host header {case} A={A} det={det}: error / bound: action {r[0]:.3f}, log-density {r[1]:.3f}")
        if det:
            np.testing.assert_allclose(logp, np.full(n, (-np.log(sd.astype(np.float64)) - ph.HALF_LOG_2PI).sum()), rtol=0, atol=(8 + A) * 2.0**-24 * (np.abs(np.log(sd.astype(np.float64))) + ph.HALF_LOG_2PI).sum())


# ------------------------------------------------------------------------------------------------------------------ c. the emulator paths

N_ENVS, T_STEPS, TRAJ = 5, 6, 4
SUB = (2, 2)      # first, count of the sub-range launch


def _spec():
    from learninghumanoidwalking_amd.envs.jvrc_walk import JvrcWalkSpec
    return JvrcWalkSpec()


def _env(spec, seed=3):
    from tests import emu
    return emu.make_emulated(spec, N_ENVS, seed=seed, max_traj_len=TRAJ, env_id_base=ENV_BASE)


def _mlp_actor(obs_dim, case, deterministic=False, counter=COUNTER0):
    """a random actor whose read-out weights are zero: mu == b3 whatever the observation"""
    from tests.test_rollout_resident import NumpyActor
    pol = NumpyActor(obs_dim, 12, seed=5, scale=2.0, deterministic=deterministic, counter=counter)
    b3, sd, exact = head_case(case, 12)
    pol.a["w3t"][:] = 0
    pol.a["b3"][:12] = b3
    pol.a["stdv"][:] = sd
    pol.view.seed = SEED
    return pol, b3, sd, exact


def _lstm_actor(obs_dim, case, deterministic=False, counter=COUNTER0):
    from tests.test_rollout_lstm import NumpyLstmActor
    pol = NumpyLstmActor(obs_dim, 12, N_ENVS, seed=5, scale=2.0, deterministic=deterministic, counter=counter)
    b3, sd, exact = head_case(case, 12)
    pol.a["wot"][:] = 0
    pol.a["bo"][:12] = b3
    pol.a["stdv"][:] = sd
    pol.view.seed = SEED
    return pol, b3, sd, exact


def _check_rollout(b, b3, sd, exact, T, counter0, rows=slice(None), deterministic=False, what=""):
    env, counter = rollout_keys(T, N_ENVS, ENV_BASE, counter0)
    return check_head(b["act"][:T, rows], b["logp"][:T, rows], b3, sd, SEED, env[:, rows], counter, exact_fma=exact, deterministic=deterministic, what=what)


def _three_launches(launch, make_actor, case, what):
    """A rollout path through its three launches: the whole batch for T = 6 control steps from counter 1000 with a truncation and an
    auto-reset inside; the sub-range first = 2, count = 2 for 2 more steps (counters 1006, 1007; the other rows stay zero); one
    deterministic step.  `launch(pol, T, first, count)` returns the rollout's buffers."""
    pol, b3, sd, exact = make_actor(case)
    b = launch(pol, T_STEPS, 0, None)
    assert (b["done"][:TRAJ] & 2).any() and np.isfinite(b["obs"]).all(), "no truncation / auto-reset inside the rollout"
    r = [_check_rollout(b, b3, sd, exact, T_STEPS, COUNTER0, what=f"{what} {case}")]
    pol.view.counter = COUNTER0 + T_STEPS
    rows = slice(SUB[0], SUB[0] + SUB[1])
    c = launch(pol, 2, *SUB)
    r.append(_check_rollout(c, b3, sd, exact, 2, COUNTER0 + T_STEPS, rows=rows, what=f"{what} {case} sub-range"))
    assert not c["act"][:, [0, 1, 4]].any() and not c["logp"][:, [0, 1, 4]].any()
    pol.view.deterministic = 1
    d = launch(pol, 1, 0, None)
    r.append(_check_rollout(d, b3, sd, exact, 1, COUNTER0 + T_STEPS, deterministic=True, what=f"{what} {case} deterministic"))
    r = np.max(r, axis=0)
    print(f"{what} {case}: error / bound: action {r[0]:.3f}, log-density {r[1]:.3f}")


@pytest.mark.parametrize("case", CASES)
def test_emulated_reference_policy_launch(case):
    """lhw_debug_policy_step (the fused strip read-out on the emulator; mlp_policy_ref_kernel where a row is wider than the strip's 64-column slab): rows
    0 .. 4 of env_id_base 4096 at counters 1000 .. 1005, narrow (37) and wide (8 x 37 = 296 columns).
    Largest error / bound: action 0.930 (dyadic) / 0.699 (random), log-density 0.025 / 0.072, the same at both widths."""
    from tests import emu
    L = emu.lib()
    rs = np.random.default_rng(2)
    for D in (37, 8 * 37):
        for det in (False, True):
            pol, b3, sd, exact = _mlp_actor(D, case, deterministic=det)
            act, logp = np.zeros((T_STEPS, N_ENVS, 12), np.float32), np.zeros((T_STEPS, N_ENVS), np.float32)
            y = np.zeros((N_ENVS, pol.view.act_pad), np.float32)
            for t in range(T_STEPS):
                obs = rs.normal(size=(N_ENVS, D)).astype(np.float32)
                rc = L.lhw_debug_policy_step(ctypes.byref(pol.view), obs.ctypes.data, N_ENVS, ENV_BASE, COUNTER0 + t, y.ctypes.data, act[t].ctypes.data,
                                             logp[t].ctypes.data, None)
                assert rc == 0, L.lhw_last_error()
                np.testing.assert_array_equal(y[:, :12], np.broadcast_to(b3, (N_ENVS, 12)))      # mu == b3
            r = _check_rollout(dict(act=act, logp=logp), b3, sd, exact, T_STEPS, COUNTER0, deterministic=det, what=f"lhw_debug_policy_step D={D} {case} det={det}")
            print(f"lhw_debug_policy_step D={D} {case} det={det}: error / bound: action {r[0]:.3f}, log-density {r[1]:.3f}")


def test_emulated_strip_read_out_keys_the_rows_of_every_workgroup():
    """lhw_debug_policy_step on 130 rows: the fused read-out of the forward strip in more than one workgroup, whose key is
    env_base + row0 + row.  Largest error / bound: action 0.881, log-density 0.094."""
    from tests import emu
    L = emu.lib()
    R = 130
    pol, b3, sd, exact = _mlp_actor(37, "random")
    obs = np.random.default_rng(4).normal(size=(R, 37)).astype(np.float32)
    act, logp, y = np.zeros((R, 12), np.float32), np.zeros(R, np.float32), np.zeros((R, pol.view.act_pad), np.float32)
    rc = L.lhw_debug_policy_step(ctypes.byref(pol.view), obs.ctypes.data, R, ENV_BASE, COUNTER0, y.ctypes.data, act.ctypes.data, logp.ctypes.data, None)
    assert rc == 0, L.lhw_last_error()
    r = check_head(act, logp, b3, sd, SEED, np.arange(R, dtype=np.uint64) + np.uint64(ENV_BASE), COUNTER0, exact_fma=exact, what="strip read-out, 130 rows")
    print(f"lhw_debug_policy_step 130 rows: error / bound: action {r[0]:.3f}, log-density {r[1]:.3f}")


@pytest.mark.parametrize("case", CASES)
def test_emulated_reference_lstm_policy_launch(case):
    """lhw_debug_lstm_policy_step (lstm_policy_ref_kernel).  Largest error / bound: action 0.930 / 0.699, log-density 0.025 / 0.072 (the keys, hence the
    figures, of lhw_debug_policy_step)."""
    from tests import emu
    L = emu.lib()
    rs = np.random.default_rng(3)
    for det in (False, True):
        pol, b3, sd, exact = _lstm_actor(37, case, deterministic=det)
        act, logp = np.zeros((T_STEPS, N_ENVS, 12), np.float32), np.zeros((T_STEPS, N_ENVS), np.float32)
        y = np.zeros((N_ENVS, pol.view.act_pad), np.float32)
        reset = np.array([1, 0, 0, 1, 0], np.uint8)
        for t in range(T_STEPS):
            obs = rs.normal(size=(N_ENVS, 37)).astype(np.float32)
            rc = L.lhw_debug_lstm_policy_step(ctypes.byref(pol.view), obs.ctypes.data, N_ENVS, reset.ctypes.data, ENV_BASE, COUNTER0 + t, y.ctypes.data,
                                              act[t].ctypes.data, logp[t].ctypes.data, None)
            assert rc == 0, L.lhw_last_error()
            np.testing.assert_array_equal(y[:, :12], np.broadcast_to(b3, (N_ENVS, 12)))
        r = _check_rollout(dict(act=act, logp=logp), b3, sd, exact, T_STEPS, COUNTER0, deterministic=det, what=f"lhw_debug_lstm_policy_step {case} det={det}")
        print(f"lhw_debug_lstm_policy_step {case} det={det}: error / bound: action {r[0]:.3f}, log-density {r[1]:.3f}")


@pytest.mark.parametrize("case", CASES)
def test_emulated_resident_rollout(case):
    """lhw_env_rollout (policy_step inside the stepper's wavefronts): the env's env_id_base, the counter advanced per control step inside the
    launch and on through an auto-reset, the sub-range's env offset, stdv[col].  Largest error / bound: action 0.950 (dyadic) / 0.760
    (random), log-density 0.025 / 0.072; the LSTM and history rollouts use the same keys and give the same figures."""
    from tests.test_rollout_resident import _resident
    spec = _spec()
    env = _env(spec)
    obs = [env.reset().copy()]

    def launch(pol, T, first, count):
        b = _resident(env, pol, T, obs[0], first=first, count=count)
        if count is None:
            obs[0] = b["obs"][T].copy()
        return b
    _three_launches(launch, lambda c: _mlp_actor(37, c), case, "lhw_env_rollout")


@pytest.mark.parametrize("case", CASES)
def test_emulated_resident_lstm_rollout(case):
    """lhw_env_rollout_lstm (lstm_policy_step).  Largest error / bound: action 0.950 / 0.760, log-density 0.025 / 0.072."""
    from tests.test_rollout_lstm import _resident
    spec = _spec()
    env = _env(spec)
    obs = [env.reset().copy()]
    reset0 = [np.ones(N_ENVS, np.uint8)]

    def launch(pol, T, first, count):
        b = _resident(env, pol, T, obs[0], reset0[0], first=first, count=count)
        if count is None:
            obs[0], reset0[0] = b["obs"][T].copy(), (b["done"][T - 1] != 0).astype(np.uint8)
        return b
    _three_launches(launch, lambda c: _lstm_actor(37, c), case, "lhw_env_rollout_lstm")


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("H", [3, 8])      # rows of 111 -> 112 columns, and of 296: past the 256 columns the in-wave step holds at a time
def test_emulated_resident_history_rollout(case, H):
    """lhw_env_rollout_history (policy_step_wide).  Largest error / bound: action 0.950 / 0.760, log-density 0.025 / 0.072."""
    from tests.test_rollout_history import _first_full, _history_env, _resident
    env = _history_env(_spec(), H, N_ENVS, seed=3, max_traj_len=TRAJ, env_id_base=ENV_BASE)
    obs = [env.reset().copy()]
    np.testing.assert_array_equal(obs[0], _first_full(obs[0][:, :37], H))

    def launch(pol, T, first, count):
        b = _resident(env, pol, T, obs[0], H, first=first, count=count)
        if count is None:
            obs[0] = b["obs"][T].copy()
        return b
    _three_launches(launch, lambda c: _mlp_actor(H * 37, c), case, f"lhw_env_rollout_history H={H}")
