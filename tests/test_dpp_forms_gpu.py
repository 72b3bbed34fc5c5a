"""The stepper's cross-lane fetches on the GPU: reference form (identity as the DPP `old` operand) against the form the kernels run (zero
identity words through bound_ctrl), lhw_debug_dpp_forms on one wavefront under five lane masks.  What is asserted and why:
tests/dpp_forms_common.py.  One launch of one wavefront per case."""
import ctypes

import numpy as np
import pytest

from tests import dpp_forms_common as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(C.MASKS))
def test_reference_and_shipped_form_move_the_same_bits(name):
    import torch
    from learninghumanoidwalking_amd import _lib
    L = _lib.lib()
    bits = C.inputs()
    x = torch.from_numpy(bits.view(np.int64)).cuda()
    out = torch.from_numpy(np.full((2, C.FORMS, 64), C.SENTINEL, np.uint64).view(np.int64)).cuda()
    _lib.check(L.lhw_debug_dpp_forms(C.MASKS[name], ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(out[0].data_ptr()), ctypes.c_void_p(out[1].data_ptr()), None))
    res = out.cpu().numpy().view(np.uint64)
    C.check(name, C.MASKS[name], bits, res[0], res[1])
