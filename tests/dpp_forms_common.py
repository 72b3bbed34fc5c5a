"""Shared by tests/test_dpp_forms_gpu.py and tests/test_dpp_forms_emu.py: inputs, lane masks and the check of lhw_debug_dpp_forms
(include/lhw.h) -- the stepper's cross-lane fetches in the reference form (identity as the DPP `old` operand) and in the form the kernels
run (zero identity words through bound_ctrl), on one wavefront under a lane mask.

What is asserted, per mask:
  * every entry of a lane outside the mask still holds the sentinel, in both outputs;
  * the two outputs are equal bit for bit -- every row, every lane of the mask -- with ONE documented exception: a row_newbcast (rbc) whose
    SOURCE lane is outside the mask.  There the hardware has nothing to fetch: the reference form returns the `old` operand, which is the
    lane's own input, bound_ctrl returns 0 (include/lhw.h; csrc/lhw_humanoid_dev.h at rbc).  No kernel reads that value; the test pins
    exactly those two values instead, which is more than leaving such lanes out;
  * both outputs equal a lane-by-lane model of the DPP controls written here from the ISA's description (row_shr / row_shl n: the lane n
    to the left / right within the 16-lane row; row_newbcast k: position k of the row; row_bcast 15 / 31: the last lane of the previous row /
    lane 31, into the rows of the row mask only), so that "equal" cannot mean "equally wrong".
These are bit moves: equality is exact, NaN payloads and the sign of zero included."""
import numpy as np

FORMS = 16                                   # include/lhw.h LHW_DPP_FORMS
SENTINEL = np.uint64(0xA5A5A5A55A5A5A5A)
ALL = (1 << 64) - 1
MASKS = {
    "all64": ALL,
    "lanes0_31": (1 << 32) - 1,                                        # a wave that serves one env in its lower half
    "rowpos0_11": sum(0xFFF << (16 * r) for r in range(4)),            # the dof lanes of every row
    "every_other": sum(1 << l for l in range(0, 64, 2)),
    "single_lane37": 1 << 37,
}
ZERO, ONE, INF = 0, 0x3FF0000000000000, 0x7FF0000000000000
_SHIFT_ROWS = [(-1, ZERO), (-2, ZERO), (-4, ZERO), (-8, ZERO), (1, ZERO), (2, ZERO), (4, ZERO), (8, ZERO), (-1, ONE), (-1, INF)]   # rows 0-9
_RBC_ROWS = {10: 0, 11: 2, 12: 5, 13: 15}


def inputs():
    """64 doubles as bits: random finite values with the special ones placed on row positions that the fetches read and fall off"""
    rng = np.random.default_rng(22)
    bits = rng.standard_normal(64).view(np.uint64).copy()
    special = {0: 0x8000000000000000,      # -0.0 at a row start (rbc<0> source)
               2: 0x0000000000000001,      # smallest denormal (rbc<2> source)
               5: 0x7FF8DEAD0000BEEF,      # NaN with a payload (rbc<5> source)
               15: 0x7FF0000000000000,     # +inf at a row end (rbc<15> source, row_bcast source)
               16: 0x000FFFFFFFFFFFFF,     # largest denormal
               31: 0xFFF0000000000000,     # -inf in lane 31 (row_bcast:31 source)
               37: 0xFFF8000000C0FFEE,     # negative NaN with a payload (the single-lane mask)
               47: 0x8000000000000000, 50: 0x7FF8DEAD0000BEEF, 63: 0x0000000000000001}
    for l, b in special.items():
        bits[l] = np.uint64(b)
    return bits


def _active(mask, l):
    return 0 <= l < 64 and (mask >> l) & 1


def model(bits, mask):
    """(ref, shipped) [FORMS][64] uint64 as the ISA describes the fetches; SENTINEL outside the mask"""
    ref = np.full((FORMS, 64), SENTINEL, np.uint64)
    lanes = [l for l in range(64) if _active(mask, l)]
    for f, (n, ident) in enumerate(_SHIFT_ROWS):
        for l in lanes:
            k = (l & 15) + n
            ref[f, l] = bits[l + n] if 0 <= k < 16 and _active(mask, l + n) else np.uint64(ident)
    shipped = ref.copy()
    for f, pos in _RBC_ROWS.items():
        for l in lanes:
            s = (l & ~15) + pos
            ref[f, l] = bits[s] if _active(mask, s) else bits[l]
            shipped[f, l] = bits[s] if _active(mask, s) else np.uint64(0)
    iv = [int((int(b) ^ (int(b) >> 32)) & 0xFFFF) for b in bits]
    for f, w in ((14, 64), (15, 32)):
        v = {l: iv[l] for l in lanes}
        for n in (1, 2, 4, 8):
            v = {l: v[l] + (v[l - n] if (l & 15) >= n and _active(mask, l - n) else 0) for l in lanes}
        v = {l: v[l] + (v[(l & ~15) - 1] if (l >> 4) in (1, 3) and _active(mask, (l & ~15) - 1) else 0) for l in lanes}      # row_bcast:15, row mask 0xa
        if w == 64:
            v = {l: v[l] + (v[31] if l >= 32 and _active(mask, 31) else 0) for l in lanes}                                  # row_bcast:31, row mask 0xc
        for l in lanes:
            ref[f, l] = shipped[f, l] = np.uint64(v[l])
    return ref, shipped


def check(name, mask, bits, ref, shipped):
    """ref / shipped: [FORMS][64] uint64 as lhw_debug_dpp_forms left them (pre-filled with SENTINEL)"""
    on = np.array([bool(_active(mask, l)) for l in range(64)])
    assert (ref[:, ~on] == SENTINEL).all() and (shipped[:, ~on] == SENTINEL).all(), f"{name}: a lane outside the mask stored"
    mref, mshipped = model(bits, mask)
    differ = np.zeros((FORMS, 64), bool)
    for f, pos in _RBC_ROWS.items():
        for l in np.flatnonzero(on):
            differ[f, l] = not _active(mask, (int(l) & ~15) + pos)
    same = ~differ
    bad = np.argwhere((ref != shipped) & same)
    assert bad.size == 0, f"{name}: reference and shipped form differ at (row, lane) {bad[:8].tolist()}: {[hex(int(ref[f, l])) for f, l in bad[:8]]} / {[hex(int(shipped[f, l])) for f, l in bad[:8]]}"
    # a row_newbcast from a lane outside the mask: own value (reference form) / 0 (bound_ctrl)
    assert (ref[differ] == np.broadcast_to(bits, (FORMS, 64))[differ]).all() and (shipped[differ] == 0).all(), f"{name}: row_newbcast from a lane outside the mask"
    assert (ref == mref).all(), f"{name}: reference form against the lane model at {np.argwhere(ref != mref)[:8].tolist()}"
    assert (shipped == mshipped).all(), f"{name}: shipped form against the lane model at {np.argwhere(shipped != mshipped)[:8].tolist()}"
