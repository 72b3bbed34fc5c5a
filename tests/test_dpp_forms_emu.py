"""CPU twin of tests/test_dpp_forms_gpu.py: lhw_debug_dpp_forms of the emulated library (the same kernel text; the emulator's OP_DPP
implements bound_ctrl, row masks and lanes that have left), under the same masks and the same assertions (tests/dpp_forms_common.py)."""
import numpy as np
import pytest

from tests import dpp_forms_common as C
from tests import emu


@pytest.mark.parametrize("name", list(C.MASKS))
def test_reference_and_shipped_form_move_the_same_bits(name):
    L = emu.lib()
    bits = C.inputs()
    x = bits.copy()
    out = np.full((2, C.FORMS, 64), C.SENTINEL, np.uint64)
    rc = L.lhw_debug_dpp_forms(C.MASKS[name], x.ctypes.data, out[0].ctypes.data, out[1].ctypes.data, None)
    assert rc == 0, L.lhw_last_error()
    C.check(name, C.MASKS[name], bits, out[0], out[1])
