"""TEST INFRASTRUCTURE: host-side SIMT emulation of the HIP stepper kernels.

`build()` compiles the product's HIP sources (csrc/lhw_humanoid.hip, lhw_cartpole.hip, lhw_api.hip) with g++
against the emulator header in this directory into tests/emu/_build/liblhw_emu.so.  The library speaks the C ABI of
include/lhw.h, so the product's own host class drives it: `make_emulated` is `spec.make_batched` with CPU tensors and
`library=lib()` -- the history bookkeeping, the choice of rollout entry point and the task shaping of
learninghumanoidwalking_amd.batched_env.BatchedEnv run in the `-m "not gpu"` suite, on top of the *kernel source* checked
against the CPU oracle (lane mappings, cross-lane reductions, LDS hand-offs, sub-wave groups) before a GPU is involved.
`EmuBatchedEnv` only adds a numpy face to reset / step / rollout / rollout_lstm.  Nothing under learninghumanoidwalking_amd/
imports this package.  Of the PPO kernels only the LDS-resident MLP strip kernels (lhw_mlp_strip.hip, f32 MFMA emulated as its
fmaf chain) are built here.
"""
from __future__ import annotations

import ctypes
import glob
import os
import subprocess

import numpy as np
import torch

from learninghumanoidwalking_amd import _lib as product
from learninghumanoidwalking_amd.batched_env import BatchedEnv

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_CSRC = os.path.join(_ROOT, "learninghumanoidwalking_amd", "csrc")
# LHW_EMU_BUILD_DIR: a build directory of its own for an instrumented library (scripts/emu_coverage.py); LHW_EMU_DEFS / LHW_EMU_LDFLAGS:
# extra words for every compile line / for the link line
_BUILD = os.environ.get("LHW_EMU_BUILD_DIR") or os.path.join(_HERE, "_build")
LIB_PATH = os.path.join(_BUILD, "liblhw_emu.so")
SOURCES = ["lhw_humanoid.hip", "lhw_humanoid_rollout.hip", "lhw_humanoid_rollout_step.hip", "lhw_cartpole.hip", "lhw_api.hip", "lhw_mlp_strip.hip"]
_LIB = None


def build(force: bool = False, opt: str = "-O1") -> str:
    srcs = [os.path.join(_CSRC, s) for s in SOURCES]
    deps = srcs + glob.glob(os.path.join(_CSRC, "*.h")) + glob.glob(os.path.join(_ROOT, "include", "*.h")) + [
        os.path.join(_HERE, "hip", "hip_runtime.h"), os.path.join(_HERE, "emu_runtime.cpp")]
    if not force and os.path.exists(LIB_PATH) and all(os.path.getmtime(LIB_PATH) >= os.path.getmtime(d) for d in deps):
        return LIB_PATH
    os.makedirs(_BUILD, exist_ok=True)
    objs = []
    procs = []
    for s in srcs + [os.path.join(_HERE, "emu_runtime.cpp")]:
        o = os.path.join(_BUILD, os.path.basename(s) + ".o")
        objs.append(o)
        cmd = ["g++", "-x", "c++", "-std=c++17", opt, "-g0", "-fPIC", "-fno-strict-aliasing", "-Wno-unused-value"] + os.environ.get("LHW_EMU_DEFS", "").split() + ["-DLHW_EMU_BUILD", "-I", _HERE,
               "-I", os.path.join(_ROOT, "include"), "-c", s, "-o", o]
        procs.append((cmd, subprocess.Popen(cmd)))
    for cmd, p in procs:
        if p.wait() != 0:
            raise RuntimeError("emulator build failed: " + " ".join(cmd))
    subprocess.check_call(["g++", "-shared", "-o", LIB_PATH] + objs + os.environ.get("LHW_EMU_LDFLAGS", "").split())
    return LIB_PATH


def lib():
    global _LIB
    if _LIB is None:
        _LIB = product.declare(ctypes.CDLL(build()))
    return _LIB


class _OnEmulator(BatchedEnv):
    """The product's BatchedEnv with device and library forced to the emulator, whatever the caller names."""

    def __init__(self, model, task, n_envs, **kw):
        super().__init__(model, task, n_envs, **dict(kw, device=torch.device("cpu"), library=lib()))


def _t(x, dtype=None):
    """the CPU tensor that shares the memory of a numpy array (None and tensors pass through)"""
    return x if x is None or isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, dtype))


class EmuBatchedEnv(_OnEmulator):
    """Numpy face of the emulated BatchedEnv for the tests written against arrays: reset / step / rollout / rollout_lstm take
    numpy arrays and return views of the env's CPU tensors.  Every other method is the product's."""

    def reset(self, mask=None):
        return super().reset(_t(mask, np.uint8)).numpy()

    def step(self, act):
        return tuple(x.numpy() for x in super().step(_t(act, np.float32).reshape(self.n_envs, self.act_dim)))

    def rollout(self, policy, T, *bufs, first=0, count=None, task_inputs=None, step_task_inputs=None):
        return super().rollout(policy, T, *map(_t, bufs), first, count, _t(task_inputs), _t(step_task_inputs))

    def rollout_lstm(self, policy, T, *bufs, first=0, count=None, task_inputs=None, step_task_inputs=None):
        return super().rollout_lstm(policy, T, *map(_t, bufs), first, count, _t(task_inputs), _t(step_task_inputs))


def make_emulated(spec, n_envs, **kw):
    """`spec.make_batched(n_envs, **kw)` on the emulated library -- built like a GPU env (YAML task shaping applied, history length
    from the spec) -- with the numpy face."""
    return numpy_face(spec.make_batched(n_envs, device=torch.device("cpu"), library=lib(), **kw))


def numpy_face(env):
    """give an emulated BatchedEnv the numpy face (methods only: the subclass owns no state)"""
    assert isinstance(env, BatchedEnv) and env.device.type == "cpu"
    env.__class__ = EmuBatchedEnv
    return env


def install_as_backend():
    """Route BatchedEnv to the emulator and make `.cuda()` a no-op (debugging aid for replaying GPU tests on a CPU)."""
    import learninghumanoidwalking_amd.batched_env as be
    be.BatchedEnv = _OnEmulator      # (make_batched looks the name up in that module at call time)
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.cuda.is_available = lambda: True
