"""CPU twin of tests/test_fastmath_gpu.py: lhw_debug_fastmath of the emulated library -- the same helper text with the seeds defined as
1.0 / x and 1.0 / sqrt(x) -- under the same inputs, bars and pinned ends (tests/fastmath_common.py).  Also holds the two references of that
module, longdouble and exact rationals, against each other."""
import numpy as np
import pytest

from tests import emu
from tests import fastmath_common as C


def test_fast_reciprocal_and_root_helpers_within_their_ulp_bars():
    L = emu.lib()
    a, b, sections = C.inputs()
    out = np.full((4, len(b)), 12345.0)
    rc = L.lhw_debug_fastmath(len(b), a.ctypes.data, b.ctypes.data, *(out[k].ctypes.data for k in range(4)), None)
    assert rc == 0, L.lhw_last_error()
    C.check(a, b, sections, dict(zip(C.OPS, out)), "emulator")


def test_bad_arguments_are_refused():
    L = emu.lib()
    x = np.ones(4)
    assert L.lhw_debug_fastmath(0, *(x.ctypes.data,) * 6, None) != 0
    assert L.lhw_debug_fastmath(4, None, *(x.ctypes.data,) * 5, None) != 0


@pytest.mark.skipif(not C.HAVE_LONGDOUBLE, reason="numpy.longdouble is a plain double here: the rational reference is the only one")
def test_longdouble_and_rational_references_agree():
    """IEEE division and sqrt as the stand-in for the helpers: under half an ulp by either reference, and the two measures equal to the
    rounding of the longdouble one (2^-11 ulp)"""
    a, b, sections = C.inputs()
    sl = sections["pos_loguniform"]
    a, b = a[sl][:300], b[sl][:300]
    for op, got in (("rcp", 1 / b), ("qdiv", a / b), ("rsqrt", 1 / np.sqrt(b)), ("qsqrt", np.sqrt(b))):
        e_ld, e_fr = C.ulp_errors_longdouble(op, a, b, got), C.ulp_errors_fraction(op, a, b, got)
        assert np.abs(e_ld - e_fr).max() < 2e-3, (op, np.abs(e_ld - e_fr).max())
        assert e_fr.max() <= (0.5 if op != "rsqrt" else 2.0)     # (1 / sqrt rounds twice: 2^-52 relative, up to 2 ulp low in a binade)
