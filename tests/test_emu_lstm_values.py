"""The critic of a stored recurrent rollout in one launch (csrc/lhw_mlp_strip.hip: lstm_seq_value_strip_kernel, behind lhw_rnn_values) on the
SIMT emulator, poison on: lhw_debug_lstm_values with fused = 1 against fused = 0 (per time slice the launches of lhw_rnn_forward's step with
a thread-per-output fmaf chain for the products).  Both run the same chains over ascending k, the same normalisation and the same cell
arithmetic, so val, vterm, vfinal and the state left behind must be EQUAL.  tests/test_lstm_values_gpu.py is the GPU twin."""
import ctypes

import numpy as np
import pytest

SENTINEL = 7.0
PAD_ROWS = 40          # rows behind every output that nobody may write (a ragged last slab has up to 31 dead rows)
STATE = ("xh1", "xh2", "c1", "c2")


def done_flags(T, N):
    """[T][N] LHW_DONE_* flags.  Column b < 32 takes pattern b % 4: no episode end; one in the middle; two at consecutive steps; one at
    t = T - 1.  Columns >= 32 (the second slab) take only the first and the last pattern, so at the middle steps that slab has no episode
    end where the first one has some.  A single column takes the last three patterns together."""
    assert T >= 4
    d = np.zeros((T, N), np.uint8)
    mid = (T - 1) // 2
    pat = {0: [], 1: [mid], 2: [mid, mid + 1], 3: [T - 1]}
    for b in range(N):
        ts = [mid, mid + 1, T - 1] if N == 1 else pat[b % 4 if b < 32 else 3 * (b % 2)]
        for t in ts:
            d[t, b] = 1 + (b + t) % 2          # terminated / truncated: both count
    return d


def done_cases(d):
    """Which of the cases the test must contain this pattern has: per-column cases, and both branches of the vterm rule."""
    T, N = d.shape
    cols = [tuple(np.flatnonzero(d[:, b])) for b in range(N)]
    slabs = [d[:, s:s + 32].any(axis=1) for s in range(0, N, 32)]
    return dict(none=any(c == () for c in cols), middle=any(any(0 < t < T - 1 for t in c) for c in cols),
                consecutive=any(any(t + 1 in c for t in c) for c in cols), at_last=any(T - 1 in c for c in cols),
                slab_step_without=any((~s).any() for s in slabs), slab_step_with=any(s.any() for s in slabs),
                same_step_both=any(any(a[t] and not b[t] for t in range(T)) for a in slabs for b in slabs))


def make_case(H, D, T, N, seed=0):
    """One network (torch's uniform(-1/sqrt(H), 1/sqrt(H)) init, scaled up so the gates leave their linear range), a stored rollout whose
    terminal observations equal the next observations except where the episode ended (what the env writes), and a non-zero state."""
    rs = np.random.default_rng(seed)
    f = np.float32
    Dp = (D + 3) & ~3
    K1 = Dp + H
    u = lambda *s: (rs.uniform(-1, 1, size=s) * 2.0 / np.sqrt(H)).astype(f)
    c = dict(H=H, D=D, Dp=Dp, T=T, N=N, w1=u(4 * H, K1), bi1=u(4 * H), bh1=u(4 * H), w2=u(4 * H, 2 * H), bi2=u(4 * H), bh2=u(4 * H),
             wo=(u(H) * 4).astype(f), bo=u(1))
    c["w1"][:, D:Dp] = SENTINEL          # the padded input columns meet zeros only
    c["obs_mean"], c["obs_std"] = rs.normal(size=D).astype(f), rs.uniform(0.5, 2.0, size=D).astype(f)
    c["obs"] = rs.normal(size=(T + 1, N, D)).astype(f)
    c["done"] = done_flags(T, N)
    tob = c["obs"][1:].copy()
    ended = c["done"] != 0
    tob[ended] = rs.normal(size=(int(ended.sum()), D)).astype(f)
    c["term_obs"] = tob
    c["reset0"] = (np.arange(N) % 3 == 1).astype(np.uint8)
    st = dict(xh1=rs.uniform(-1, 1, size=(N, K1)), xh2=rs.uniform(-1, 1, size=(N, 2 * H)), c1=rs.normal(size=(N, H)), c2=rs.normal(size=(N, H)))
    c["state"] = {k: v.astype(f) for k, v in st.items()}
    return c


def state_columns(c, st):
    """The four state buffers proper: the recurrent columns of xh1 / xh2, and c1 / c2 (all rows, guard rows included)."""
    return dict(h1=st["xh1"][:, c["Dp"]:], h2=st["xh2"][:, c["H"]:], c1=st["c1"], c2=st["c2"])


def run_values(L, c, fused, t0=0, t1=None, state=None, reset0="case", want_term=True, want_final=True, ptr=lambda a: a.ctypes.data, alloc=None,
               dev=lambda a: a, host=np.asarray):
    """One call over the steps [t0, t1) of the case on sentinel-guarded buffers, from `state` (default: the case's initial state).
    `alloc(shape, dtype, fill)` / `ptr` / `dev` / `host` let the GPU twin run the same steps on device buffers.  Returns host arrays
    val, vterm, vfinal (each with PAD_ROWS guard entries) and the state dict (guard rows included)."""
    from learninghumanoidwalking_amd._lib import LhwLstmValuesArgs
    alloc = alloc or (lambda shape, dt, fill: np.full(shape, fill, dt))
    H, D, Dp, N = c["H"], c["D"], c["Dp"], c["N"]
    t1 = c["T"] if t1 is None else t1
    T = t1 - t0
    f = np.float32
    st = {}
    for k, v in (state or c["state"]).items():
        g = np.full((N + PAD_ROWS, v.shape[1]), SENTINEL, f)
        g[:N] = v[:N]
        st[k] = dev(g)
    out = dict(val=alloc((T * N + PAD_ROWS,), f, SENTINEL), vterm=alloc((T * N + PAD_ROWS,), f, SENTINEL), vfinal=alloc((N + PAD_ROWS,), f, SENTINEL))
    scratch = alloc((max((Dp + 3 * H) * 4 * H, 6 * N * H),), f, SENTINEL)
    r0 = c["reset0"] if isinstance(reset0, str) else reset0
    keep = {k: dev(np.ascontiguousarray(c[k])) for k in ("w1", "bi1", "bh1", "w2", "bi2", "bh2", "wo", "bo", "obs_mean", "obs_std")}
    keep.update(obs=dev(np.ascontiguousarray(c["obs"][t0:t1 + 1])), term_obs=dev(np.ascontiguousarray(c["term_obs"][t0:t1])),
                done=dev(np.ascontiguousarray(c["done"][t0:t1])), reset0=dev(np.ascontiguousarray(r0)))
    a = LhwLstmValuesArgs(H=H, D=D, Dp=Dp, T=T, N=N, scratch=ptr(scratch), **{k: ptr(v) for k, v in keep.items()}, **{k: ptr(v) for k, v in st.items()},
                          **{k: ptr(v) for k, v in out.items()})
    if not want_term:
        a.term_obs = a.vterm = None
    if not want_final:
        a.vfinal = None
    assert L.lhw_debug_lstm_values(ctypes.byref(a), int(fused), None) == 0, L.lhw_last_error()
    return {k: host(v) for k, v in out.items()}, {k: host(v) for k, v in st.items()}


def check_equal(c, ref, got, T=None, want_term=True, want_final=True):
    """`got` against `ref` (each: outputs, state): equal everywhere, every live entry written, no guard entry touched."""
    N = c["N"]
    R = (c["T"] if T is None else T) * N
    (ro, rst), (go, gst) = ref, got
    for k, n, on in (("val", R, True), ("vterm", R, want_term), ("vfinal", N, want_final)):
        if on:
            assert np.isfinite(go[k][:n]).all() and (go[k][:n] != SENTINEL).all(), f"{k}: entry never written"
            assert np.array_equal(ro[k], go[k]), f"{k}: {np.flatnonzero(ro[k] != go[k])[:8]}, max |diff| = {np.abs(ro[k][:n] - go[k][:n]).max():.3e}"
        assert (go[k][n if on else 0:] == SENTINEL).all(), f"{k}: entries beyond the rollout must not be written"
    for (k, a), b in zip(state_columns(c, rst).items(), state_columns(c, gst).values()):
        assert np.isfinite(b[:N]).all() and (b[N:] == SENTINEL).all(), f"{k}: guard rows"
        assert np.array_equal(a, b), f"{k}: max |diff| = {np.abs(a[:N] - b[:N]).max():.3e}"


# H = 32: one wave per workgroup; H = 64: two, the units split across waves.  D = 5: Dp = 8, padded columns.  N = 40: a full slab and a ragged one
# of 8 rows; N = 1.
CASES = [pytest.param(dict(H=32, D=5, T=5, N=40), id="h32-n40"), pytest.param(dict(H=64, D=5, T=5, N=40), id="h64-n40"),
         pytest.param(dict(H=32, D=5, T=5, N=1), id="h32-n1"), pytest.param(dict(H=64, D=5, T=5, N=1), id="h64-n1")]


def test_done_patterns_are_what_the_cases_claim():
    many, one = done_cases(done_flags(5, 40)), done_cases(done_flags(5, 1))
    assert all(many.values()), many
    assert all(v for k, v in one.items() if k not in ("none", "same_step_both")), one
    assert not done_cases(np.zeros((5, 40), np.uint8))["slab_step_with"] and not done_cases(np.ones((5, 40), np.uint8))["slab_step_without"]
    c = make_case(32, 5, 5, 40)
    ended = c["done"] != 0
    assert np.array_equal(c["term_obs"][~ended], c["obs"][1:][~ended]) and (c["term_obs"][ended] != c["obs"][1:][ended]).any(axis=1).all()
    assert c["reset0"].any() and not c["reset0"].all() and all(np.abs(v).min() > 0 for v in c["state"].values())


@pytest.mark.parametrize("kw", CASES)
def test_value_strip_equals_the_per_step_calls_on_the_emulator(kw):
    from tests import emu
    L = emu.lib()
    c = make_case(seed=3, **kw)
    ref, got = run_values(L, c, fused=0), run_values(L, c, fused=1)
    check_equal(c, ref, got)
    # the reference is not trivially flat: the terminal values differ from the next values exactly where episodes ended
    N, T = c["N"], c["T"]
    val, vterm, ended = got[0]["val"][:T * N].reshape(T, N), got[0]["vterm"][:T * N].reshape(T, N), c["done"] != 0
    assert (vterm[:-1][ended[:-1]] != val[1:][ended[:-1]]).all() and np.array_equal(vterm[:-1][~ended[:-1]], val[1:][~ended[:-1]])
    assert np.array_equal(vterm[-1][~ended[-1]], got[0]["vfinal"][:N][~ended[-1]])


@pytest.mark.parametrize("kw", CASES[1:3])
def test_value_strip_carries_its_state_from_call_to_call(kw):
    """T = 5 in one call == 2 + 3 steps in two calls (the second one's reset0 = the first one's last done flags)."""
    from tests import emu
    L = emu.lib()
    c = make_case(seed=4, **kw)
    N, T = c["N"], c["T"]
    whole = run_values(L, c, fused=1)
    o1, s1 = run_values(L, c, fused=1, t0=0, t1=2)
    o2, s2 = run_values(L, c, fused=1, t0=2, t1=T, state=s1, reset0=(c["done"][1] != 0).astype(np.uint8))
    for k in ("val", "vterm"):
        assert np.array_equal(np.concatenate([o1[k][:2 * N], o2[k][:3 * N]]), whole[0][k][:T * N]), k
    assert np.array_equal(o2["vfinal"], whole[0]["vfinal"])
    for (k, a), b in zip(state_columns(c, whole[1]).items(), state_columns(c, s2).values()):
        assert np.array_equal(a, b), k
    # and against the per-step reference run the same way
    check_equal(c, run_values(L, c, fused=0, t0=2, t1=T, state=s1, reset0=(c["done"][1] != 0).astype(np.uint8)), (o2, s2), T=3)


def test_value_strip_without_terminal_and_final_values():
    from tests import emu
    L = emu.lib()
    c = make_case(32, 5, 5, 40, seed=6)
    kw = dict(want_term=False, want_final=False)
    check_equal(c, run_values(L, c, fused=0, **kw), run_values(L, c, fused=1, **kw), **kw)
    kw = dict(want_term=True, want_final=False)
    check_equal(c, run_values(L, c, fused=0, **kw), run_values(L, c, fused=1, **kw), **kw)


def test_value_strip_refuses_what_it_cannot_hold():
    from learninghumanoidwalking_amd._lib import LhwLstmValuesArgs
    from tests import emu
    L = emu.lib()
    z = np.zeros(64, np.float32)
    names = [n for n, _ in LhwLstmValuesArgs._fields_ if n not in ("H", "D", "Dp", "T", "N")]
    for H, Dp in ((48, 40), (288, 40), (64, 132)):
        a = LhwLstmValuesArgs(H=H, D=Dp, Dp=Dp, T=1, N=1, **{k: z.ctypes.data for k in names})
        assert L.lhw_debug_lstm_values(ctypes.byref(a), 1, None) == -4      # LHW_ERR_UNSUPPORTED
