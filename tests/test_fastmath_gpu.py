"""The stepper's fp64 reciprocal / division / square-root helpers on the hardware: v_rcp_f64 / v_rsq_f64 plus two Newton steps
(csrc/lhw_humanoid_dev.h), lhw_debug_fastmath in one launch over a few thousand input pairs, against a wider reference.  Inputs, bars and the
pinned non-IEEE ends: tests/fastmath_common.py; tests/test_fastmath_emu.py is the emulator's twin."""
import ctypes

import numpy as np
import pytest

from tests import fastmath_common as C

pytestmark = pytest.mark.gpu


def test_fast_reciprocal_and_root_helpers_within_their_ulp_bars():
    import torch
    from learninghumanoidwalking_amd import _lib
    L = _lib.lib()
    a, b, sections = C.inputs()
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    out = torch.full((4, len(b)), 12345.0, dtype=torch.float64, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.check(L.lhw_debug_fastmath(len(b), p(da), p(db), p(out[0]), p(out[1]), p(out[2]), p(out[3]), None))
    torch.cuda.synchronize()
    C.check(a, b, sections, dict(zip(C.OPS, out.cpu().numpy())), "gfx950")
