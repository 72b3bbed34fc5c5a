"""Shared by tests/test_policy_head.py (CPU: the header compiled for the host, the SIMT emulator) and tests/test_policy_head_gpu.py:
the two parameter cases of the Gaussian head and the pointwise bounds that hold a sampled action and its stored log-density to the
float64 restatement (oracle/policy_head.py).  Not a test module.

The bounds are derived from the arithmetic lhw_policy.h documents, not tuned.  With z64, mu, sd the restatement's values for a key:

  action       |act - (mu + sd z64)| <= 2^-24 |act| + sd (2^-24 |z64| + 1e-13)
               one fmaf rounding (half an ulp of the result), one rounding of z to float32, and 1e-13 for the few-ulp differences
               between the double log / cos of the device, glibc and numpy (|z| <= 8.6).  Where mu == 0 and sd is a power of two
               the fmaf is exact and the first term is dropped (`exact_fma`).
  log-density  against log_density64 of the STORED float32 action:  |logp - ref| <= (8 + A) 2^-24 S,
               S = sum_a (d_a^2 / 2 + |log sd_a| + 0.9189...): at most 8 half-ulp relative errors per term (subtract, divide, square,
               logf, two adds) plus the A-term ascending float32 sum.  A wrong constant or a missing 1/2 is an O(1) multiple of S.

A wrong key (env, counter, slot, stream) moves z by O(1): about 1e7 bounds."""
import numpy as np

from oracle import policy_head as ph

EPS = 2.0 ** -24
SEED = 2**63 + 1234567          # (>= 2**63: a seed that is negative as an int64)
ENV_BASE = 4096
COUNTER0 = 1000


def head_case(name, A, rs_seed=0):
    """(b3 [A], sd [A], exact_fma) float32.  'dyadic': b3 = 0 and power-of-two stds 1/16 .. 2, neighbours distinct, so act == sd * z with
    no rounding besides z's; 'random': b3 random, stds non-dyadic and all distinct in [0.05, 2]."""
    rs = np.random.default_rng(1000 + rs_seed + A)
    if name == "dyadic":
        return np.zeros(A, np.float32), (2.0 ** ((np.arange(A) % 6) - 4.0)).astype(np.float32), True
    assert name == "random"
    sd = rs.uniform(0.05, 2.0, size=A).astype(np.float32)
    assert len(set(sd.tolist())) == A
    return (rs.normal(size=A) * 0.3).astype(np.float32), sd, False


CASES = ("dyadic", "random")


def check_head(act, logp, mu, sd, seed, env, counter, *, exact_fma=False, deterministic=False, what=""):
    """act [..., A], logp [...] float32 from the code under test; mu [..., A] (or [A]) and sd [A] the float32 parameters it was given;
    env, counter: integer arrays broadcastable to logp's shape (GLOBAL env index, step counter).  Asserts the module's bounds and
    returns the largest (action error / bound, log-density error / bound)."""
    act, logp = np.asarray(act), np.asarray(logp)
    assert act.dtype == np.float32 and logp.dtype == np.float32, (act.dtype, logp.dtype)
    A = act.shape[-1]
    assert logp.shape == act.shape[:-1]
    mu = np.broadcast_to(np.asarray(mu, np.float32), act.shape).astype(np.float64)
    sd = np.asarray(sd, np.float32).astype(np.float64)
    assert sd.shape == (A,)
    env = np.broadcast_to(np.asarray(env, np.uint64), logp.shape)
    counter = np.broadcast_to(np.asarray(counter, np.uint64), logp.shape)
    assert np.isfinite(act).all() and np.isfinite(logp).all(), what
    a64 = act.astype(np.float64)
    if deterministic:
        np.testing.assert_array_equal(a64, mu, err_msg=f"{what}: a deterministic action is the mean")
        r_act = 0.0
    else:
        seed = np.broadcast_to(np.asarray(seed, np.uint64), logp.shape)
        z = ph.normal64(seed[..., None], env[..., None], counter[..., None], np.arange(A, dtype=np.uint64))
        want = mu + sd * z      # (= ph.sample64(mu, sd, seed, env, counter))
        err = np.abs(a64 - want)
        bound = (0.0 if exact_fma else EPS * np.abs(a64)) + sd * (EPS * np.abs(z) + 1e-13)
        r_act = float((err / bound).max())
        i = np.unravel_index(np.argmax(err / bound), err.shape)
        assert r_act <= 1.0, f"{what}: action {i}: {a64[i]!r} vs {want[i]!r} (z64 = {z[i]!r}), error / bound = {r_act:.3g}"
    ref = ph.log_density64(a64, mu, sd)
    S = ph.log_density_scale(a64, mu, sd)
    lerr = np.abs(logp.astype(np.float64) - ref) / ((8 + A) * EPS * S)
    r_lp = float(lerr.max()) if lerr.size else 0.0
    i = np.unravel_index(np.argmax(lerr), lerr.shape) if lerr.size else ()
    assert r_lp <= 1.0, f"{what}: log-density {i}: {logp[i]!r} vs {ref[i]!r} (S = {S[i]:.4g}), error / bound = {r_lp:.3g}"
    return r_act, r_lp


def rollout_keys(T, N, env_base=ENV_BASE, counter0=COUNTER0):
    """(env [1][N], counter [T][1]) of a rollout's [T][N] rows"""
    return (np.arange(N, dtype=np.uint64)[None, :] + np.uint64(env_base), np.arange(T, dtype=np.uint64)[:, None] + np.uint64(counter0))
