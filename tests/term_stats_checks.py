"""Shared checks of the per-term episode statistics (lhw_env_enable_term_stats / lhw_env_pop_term_stats, include/lhw.h) for
tests/test_term_stats.py (SIMT emulator) and tests/test_term_stats_gpu.py: the host recomputation that segments per-step reward terms
by the done flags, and the bounds.  The reference keeps these numbers as the `info` dictionary of every env.step
(/root/reference/robots/robot_base.py:88-96); a batched rollout drops them unless the kernels accumulate them."""
import ctypes

import numpy as np

F32_EPS = 2.0 ** -23      # bound of check 3: |device - host| <= 2^-23 * sum |term| (each read-back term was rounded to float32 once)
ORDER_RTOL = 1e-9         # checks 4 / 5: the same float64 numbers added in another order (n * eps for <= 1e4 additions is 1e-12)


def enable(env, on=True):
    env.enable_term_stats(on)


def pop(env):
    """(term sums [n_terms], episodes, terminated, truncated): the raw call, for the library's own `episodes` counter -- BatchedEnv.pop_term_sums
    returns the two kinds of ending only, and check_counts holds the three numbers against each other"""
    s = np.zeros(env.n_terms)
    ep, te, tr = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    rc = env._L.lhw_env_pop_term_stats(env._h, s.ctypes.data, ctypes.byref(ep), ctypes.byref(te), ctypes.byref(tr))
    assert rc == 0, env._L.lhw_last_error()
    return s, ep.value, te.value, tr.value


def counts_from_done(done):
    """(episodes, terminated, truncated) the [T][N] flag buffer reports: bit 0 terminated, bit 1 alone truncated"""
    d = np.asarray(done)
    return int((d != 0).sum()), int(((d & 1) != 0).sum()), int((d == 2).sum())


def host_term_sums(terms, done, carry=None):
    """Segment per-step terms [T][N][K] (float32 read-backs, summed here in float64) by done [T][N].
    Returns (sum over finished episodes [K], sum of |term| over the steps of those episodes [K], carry [N][K] of the running episodes,
    carry of |term| [N][K])."""
    T, N, K = terms.shape
    run = np.zeros((N, K)) if carry is None else carry[0].copy()
    run_abs = np.zeros((N, K)) if carry is None else carry[1].copy()
    fin, fin_abs = np.zeros(K), np.zeros(K)
    for t in range(T):
        x = terms[t].astype(np.float64)
        run += x
        run_abs += np.abs(x)
        for n in np.nonzero(done[t])[0]:
            fin += run[n]
            fin_abs += run_abs[n]
            run[n] = 0
            run_abs[n] = 0
    return fin, fin_abs, (run, run_abs)


def check_counts(popped, done, ep_count):
    """check 2: exact counts"""
    _, ep, te, tr = popped
    want = counts_from_done(done)
    print("counts device (episodes, terminated, truncated)", (ep, te, tr), "done buffer", want, "episode stats", ep_count)
    assert (ep, te, tr) == want
    assert ep == ep_count and te + tr == ep


def check_against_host(popped, host_sum, host_abs):
    """check 3: device float64 sums vs the host's sums of the float32 read-backs"""
    err = np.abs(popped[0] - host_sum)
    bound = F32_EPS * host_abs
    print("term sums: max |device - host| / bound", float((err / np.maximum(bound, 1e-300)).max()), "err", err, "bound", bound)
    assert (err <= bound).all(), (err, bound)


def check_same_up_to_order(a, b, what):
    """checks 4 / 5: two float64 sums of the same numbers"""
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    tol = ORDER_RTOL * max(np.abs(a).sum(), np.abs(b).sum())
    print(what, "max |a - b|", float(np.abs(a - b).max()), "tol", tol)
    assert (np.abs(a - b) <= tol).all(), (what, a, b)


def check_zero(popped):
    s, ep, te, tr = popped
    assert not s.any() and (ep, te, tr) == (0, 0, 0), popped
