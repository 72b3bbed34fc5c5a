"""TEST INFRASTRUCTURE: lhw_video.hip on the host-side SIMT emulator.

tests.emu.build() compiles the stepper's sources against tests/emu/hip/hip_runtime.h; this helper compiles lhw_video.hip with the same
g++ line and links it with those objects into a library of its own, tests/emu/_build/liblhw_emu_video.so, so that
`JpegEncoder(..., device="cpu", library=lib())` runs the kernel source -- the lane-per-block passes, the prefix sums, the bit buffer, the
ballot of the byte stuffing -- on CPU tensors.
"""
import ctypes
import os
import subprocess

from learninghumanoidwalking_amd import _lib as product
from tests import emu

_SRC = os.path.join(emu._CSRC, "lhw_video.hip")
LIB_PATH = os.path.join(emu._BUILD, "liblhw_emu_video.so")
_LIB = None


def build(force: bool = False, opt: str = "-O1") -> str:
    base = emu.build()
    deps = [base, _SRC, os.path.join(emu._CSRC, "lhw_internal.h"), os.path.join(emu._ROOT, "include", "lhw.h"), os.path.abspath(__file__)]
    if not force and os.path.exists(LIB_PATH) and all(os.path.getmtime(LIB_PATH) >= os.path.getmtime(d) for d in deps):
        return LIB_PATH
    obj = os.path.join(emu._BUILD, "lhw_video.hip.o")
    subprocess.check_call(["g++", "-x", "c++", "-std=c++17", opt, "-g0", "-fPIC", "-fno-strict-aliasing", "-Wno-unused-value"] +
                          os.environ.get("LHW_EMU_DEFS", "").split() + ["-DLHW_EMU_BUILD", "-I", emu._HERE, "-I", os.path.join(emu._ROOT, "include"),
                                                                        "-c", _SRC, "-o", obj])
    objs = [os.path.join(emu._BUILD, os.path.basename(s) + ".o") for s in emu.SOURCES + ["emu_runtime.cpp"]] + [obj]
    tmp = LIB_PATH + f".{os.getpid()}.tmp"
    subprocess.check_call(["g++", "-shared", "-o", tmp] + objs + os.environ.get("LHW_EMU_LDFLAGS", "").split())
    os.replace(tmp, LIB_PATH)
    return LIB_PATH


def lib():
    global _LIB
    if _LIB is None:
        _LIB = product.declare(ctypes.CDLL(build()))
    return _LIB
