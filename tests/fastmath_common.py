"""Shared by tests/test_fastmath_gpu.py and tests/test_fastmath_emu.py: inputs, reference and checks of lhw_debug_fastmath (include/lhw.h)
-- rcp_f64, qdiv, rsqrt_f64 and qsqrt of csrc/lhw_humanoid_dev.h, the seed instruction (v_rcp_f64 / v_rsq_f64; on the emulator 1.0 / x and
1.0 / sqrt(x)) plus two Newton steps, in one launch over a few thousand input pairs.

Reference: the same operation in numpy.longdouble where that has a 64-bit mantissa (x86), else exact rational arithmetic
(fractions.Fraction, math.isqrt for the roots); the two are held against each other in tests/test_fastmath_emu.py.

Bars, in ulps of the reference's binade (2^(e - 52) for 2^e <= |ref| < 2^(e + 1); a reference that is exactly 2^e takes the ulp of the
binade above it, the larger of the two candidates, which only matters for an error of zero):
rcp_f64, rsqrt_f64, qsqrt 2 ulp, qdiv 3 ulp.  Once the Newton steps have converged the last fma rounds once (under 1 ulp of its own
result), the product a * x of qdiv adds half an ulp, and an ulp's relative size varies by a factor of two across a binade.

The ends are NOT IEEE and are pinned as the helpers return them today (ENDS below): the first fma of a Newton step sees 0 * inf."""
import math
from fractions import Fraction

import numpy as np

HMINVAL = 1e-15                              # csrc/lhw_humanoid_dev.h
BARS = {"rcp": 2.0, "qdiv": 3.0, "rsqrt": 2.0, "qsqrt": 2.0}
OPS = ("rcp", "qdiv", "rsqrt", "qsqrt")
HAVE_LONGDOUBLE = np.finfo(np.longdouble).nmant >= 63

# (a, b) -> class of (rcp_f64(b), qdiv(a, b), rsqrt_f64(b), qsqrt(b)); IEEE would give +-inf for x / 0, 0 for x / inf, inf for 1 / sqrt(0)
# and inf for sqrt(inf)
_INF, _NAN = float("inf"), float("nan")
ENDS = [
    (1.0, 0.0, ("nan", "nan", "nan", "+zero")),
    (1.0, -0.0, ("nan", "nan", "nan", "+zero")),
    (-3.0, _INF, ("nan", "nan", "nan", "nan")),
    (2.0, -_INF, ("nan", "nan", "nan", "nan")),
    (1.0, _NAN, ("nan", "nan", "nan", "nan")),
    (_NAN, 2.0, ("finite", "nan", "finite", "finite")),
    (0.0, 2.0, ("finite", "+zero", "finite", "finite")),
    (-0.0, 2.0, ("finite", "-zero", "finite", "finite")),
    (0.0, -2.0, ("finite", "-zero", "nan", "nan")),
    (_INF, 4.0, ("finite", "+inf", "finite", "finite")),
    (_INF, -4.0, ("finite", "-inf", "nan", "nan")),
    (0.0, 0.0, ("nan", "nan", "nan", "+zero")),
]
# radicands below anything a call site forms from squared lengths short of underflow to 0: qsqrt stays finite (and positive) down to the
# smallest denormal
TINY = [5e-324, 2.5e-320, 2.2250738585072014e-308, 1e-300, 1e-200, HMINVAL * HMINVAL * 1e-30]


def inputs():
    """(a, b, sections): float64 arrays and {name: slice}.  Sections `pos*`: b > 0, all four results against the reference; `neg`: b < 0,
    the divisions against the reference and NaN roots; `ends` / `tiny`: ENDS / TINY."""
    rng = np.random.default_rng(25)
    parts, sections, at = [], {}, 0

    def add(name, a, b):
        nonlocal at
        a, b = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64))
        parts.append((a.ravel(), b.ravel()))
        sections[name] = slice(at, at + a.size)
        at += a.size

    def loguniform(n):
        return 10.0 ** rng.uniform(-30, 30, n)

    add("pos_loguniform", loguniform(1500) * rng.choice([-1.0, 1.0], 1500), loguniform(1500))
    add("neg", loguniform(500) * rng.choice([-1.0, 1.0], 500), -loguniform(500))
    # around powers of two: 2^k and the four doubles on either side, k = -100 .. 100
    p2 = []
    for k in range(-100, 101):
        lo = hi = math.ldexp(1.0, k)
        p2.append(lo)
        for _ in range(4):
            lo, hi = np.nextafter(lo, 0.0), np.nextafter(hi, np.inf)
            p2 += [lo, hi]
    add("pos_pow2", loguniform(len(p2)) * rng.choice([-1.0, 1.0], len(p2)), p2)
    # 1 +- k 2^-52 (1 - k 2^-53 below one), k = 0 .. 64, and every 1/256 of the binade with two doubles on either side: where a seed table
    # indexed by the leading mantissa bits steps
    near1 = [1.0 + k * 2.0 ** -52 for k in range(65)] + [1.0 - k * 2.0 ** -53 for k in range(1, 65)] + [1.0 - k * 2.0 ** -52 for k in range(1, 65)]
    steps = [1.0 + m / 256.0 + j * 2.0 ** -52 for m in range(1, 256) for j in (-2, -1, 0, 1, 2)]
    add("pos_near1", 1.0, near1)
    add("pos_table", rng.uniform(0.5, 2.0, len(steps)), steps)
    add("pos_table_x2", rng.uniform(0.5, 2.0, len(steps)), 2.0 * np.asarray(steps))     # the odd-exponent half of the rsq table
    # what the call sites produce: HMINVAL pivots and regularisers, HMINVAL^2, 1 - R^2 of nearly parallel capsule axes down to 1e-12,
    # masses / inertias (meaninertia-scale), time constants and gears; numerators 1, 2 and a unit-length component
    site = [HMINVAL, HMINVAL * HMINVAL, np.nextafter(HMINVAL, 1.0), np.nextafter(HMINVAL * HMINVAL, 1.0)]
    site += [1.0 - (1.0 - 10.0 ** -k) ** 2 for k in range(1, 13)] + [10.0 ** -k for k in range(0, 13)]
    site += [0.0005, 0.002, 0.005, 0.02, 0.9, 0.95, 0.001, 0.5, 2.0, 0.05, 0.38, 1.3, 4.7, 9.81, 17.0, 41.4, 62.0, 100.0, 2.44]
    site += list(rng.uniform(0.001, 60.0, 64))
    for num in (1.0, 2.0, -0.7071067811865476):
        add(f"pos_site_{num:g}", num, site)
    add("ends", [e[0] for e in ENDS], [e[1] for e in ENDS])
    add("tiny", 1.0, TINY)
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), sections


def _ulp_of(ref):
    """the ulp of float64 in the binade of |ref| (longdouble array, nonzero finite)"""
    _, e = np.frexp(np.abs(ref))                   # |ref| = m 2^e, 0.5 <= m < 1
    return np.ldexp(np.longdouble(1.0), e - 53)


def ulp_errors_longdouble(op, a, b, got):
    ld = np.longdouble
    a, b, got = a.astype(ld), b.astype(ld), got.astype(ld)
    ref = {"rcp": lambda: 1 / b, "qdiv": lambda: a / b, "rsqrt": lambda: 1 / np.sqrt(b), "qsqrt": lambda: np.sqrt(b)}[op]()
    return (np.abs(got - ref) / _ulp_of(ref)).astype(np.float64)


def _sqrt_fraction(x: Fraction, bits: int = 160) -> Fraction:
    """sqrt(x) to a relative 2^-bits, rounded down"""
    p, q = x.numerator, x.denominator
    return Fraction(math.isqrt(p * q << (2 * bits)), q << bits)


def ulp_errors_fraction(op, a, b, got):
    out = np.empty(len(b))
    for i, (x, d, g) in enumerate(zip(a.tolist(), b.tolist(), got.tolist())):
        if not math.isfinite(g):
            out[i] = math.inf
            continue
        x, d = Fraction(x), Fraction(d)
        ref = {"rcp": lambda: 1 / d, "qdiv": lambda: x / d, "rsqrt": lambda: 1 / _sqrt_fraction(d), "qsqrt": lambda: _sqrt_fraction(d)}[op]()
        n = abs(ref)
        e = n.numerator.bit_length() - n.denominator.bit_length()              # 2^(e-1) < n < 2^(e+1)
        e = e if n >= Fraction(2) ** e else e - 1                              # 2^e <= n < 2^(e+1)
        out[i] = float(abs(Fraction(g) - ref) / Fraction(2) ** (e - 52))
    return out


ulp_errors = ulp_errors_longdouble if HAVE_LONGDOUBLE else ulp_errors_fraction


def classify(x):
    if math.isnan(x):
        return "nan"
    if math.isinf(x):
        return "+inf" if x > 0 else "-inf"
    if x == 0.0:
        return "-zero" if math.copysign(1.0, x) < 0 else "+zero"
    return "finite"


def check(a, b, sections, res, where):
    """res: {op: float64 [n]} as lhw_debug_fastmath left them.  Prints the measured maxima (ulp) per helper, then asserts the bars, the
    NaN roots of negative radicands, the ends and the tiny radicands.  Returns the maxima."""
    pos = np.zeros(len(b), bool)
    for name, sl in sections.items():
        if name.startswith("pos"):
            pos[sl] = True
    assert (b[pos] > 0).all() and pos.sum() >= 3000
    div = pos.copy()
    div[sections["neg"]] = True
    worst = {}
    for op in OPS:
        sel = div if op in ("rcp", "qdiv") else pos
        assert np.isfinite(res[op][sel]).all(), (where, op, "non-finite result for a finite nonzero input")
        err = ulp_errors(op, a[sel], b[sel], res[op][sel])
        i = int(np.argmax(err))
        worst[op] = (float(err[i]), float(a[sel][i]), float(b[sel][i]))
        print(f"fastmath[{where}] {op}: max {err[i]:.4f} ulp at a = {a[sel][i]!r}, b = {b[sel][i]!r}; mean {err.mean():.4f} ulp over {sel.sum()} inputs")
    for op in OPS:
        assert worst[op][0] <= BARS[op], (where, op, worst[op], "ulp, a, b")
    neg = sections["neg"]
    assert np.isnan(res["rsqrt"][neg]).all() and np.isnan(res["qsqrt"][neg]).all()
    ends = sections["ends"]
    for k, (ea, eb, want) in enumerate(ENDS):
        got = tuple(classify(float(res[op][ends][k])) for op in OPS)
        assert got == want, (where, "a, b", ea, eb, "got", got, "pinned", want)
    tiny = res["qsqrt"][sections["tiny"]]
    assert np.isfinite(tiny).all() and (tiny > 0).all(), tiny
    t = np.asarray(TINY)
    normal = t >= 2.2250738585072014e-308
    assert (ulp_errors("qsqrt", t[normal], t[normal], tiny[normal]) <= BARS["qsqrt"]).all()
    return worst
