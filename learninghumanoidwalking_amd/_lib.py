"""ctypes loader for liblhw.so (the C ABI in include/lhw.h).  No CPU fallback: if the
library is missing or no GPU is visible, calls fail loudly."""
from __future__ import annotations

import ctypes
import glob
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
LIB_PATH = os.environ.get("LHW_LIB") or os.path.join(_HERE, "liblhw.so")   # LHW_LIB: kernel-variant experiments (scripts/)
_LIB = None


class LhwError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"liblhw error {code}: {msg}")
        self.code = code


class LhwEnvConfig(ctypes.Structure):
    _fields_ = [
        ("task", ctypes.c_int32), ("n_envs", ctypes.c_int32), ("device", ctypes.c_int32),
        ("frame_skip", ctypes.c_int32), ("max_traj_len", ctypes.c_int32), ("env_id_base", ctypes.c_int32),
        ("seed", ctypes.c_uint64), ("action_smoothing", ctypes.c_double),
        ("kp", ctypes.c_void_p), ("kd", ctypes.c_void_p), ("nominal_qpos", ctypes.c_void_p),
        ("action_offset", ctypes.c_void_p), ("task_params", ctypes.c_void_p), ("n_task_params", ctypes.c_int32),
        ("task_iparams", ctypes.c_void_p), ("n_task_iparams", ctypes.c_int32),
        ("clock_lut", ctypes.c_void_p), ("period", ctypes.c_int32), ("init_noise", ctypes.c_double),
        ("perturb_interval", ctypes.c_int32), ("n_perturb_bodies", ctypes.c_int32), ("perturb_bodies", ctypes.c_int32 * 2),
        ("perturb_force", ctypes.c_double), ("perturb_torque", ctypes.c_double),
    ]


TASK_CARTPOLE, TASK_JVRC_WALK, TASK_H1_STAND, TASK_JVRC_STEP, TASK_H1_WALK = 0, 1, 2, 3, 4      # include/lhw.h: LhwEnvConfig.task

# The reward dictionary of each task in the reference's dict order -- the order of rew_terms, of lhw_env_pop_term_stats and of
# lhw_env_set_task_shaping (cartpole_env.py:182-187, walking_task.py:131-146, standing_task.py:99-106, stepping_task.py:109-122)
_WALK_TERMS = ("foot_frc_score", "foot_vel_score", "root_accel", "height_error", "com_vel_error", "yaw_vel_error", "upper_body_reward",
               "posture_error", "torque_penalty", "action_penalty")
REWARD_TERMS = {TASK_CARTPOLE: ("upright", "center", "velocity", "action"), TASK_JVRC_WALK: _WALK_TERMS, TASK_H1_WALK: _WALK_TERMS,
                TASK_H1_STAND: ("com_vel_error", "yaw_vel_error", "height", "upperbody", "joint_torque_reward", "posture"),
                TASK_JVRC_STEP: ("foot_frc_score", "foot_vel_score", "orient_cost", "height_error", "step_reward", "upper_body_reward")}
# Task shaping an env starts with -- the reference's literals, as humanoid_create fills them (lhw_env_get_task_shaping on a fresh env
# returns these; tests/test_task_shaping.py holds the two tables together): term weights in REWARD_TERMS order, and the termination
# bounds (lo, hi) on the root height (stepping task: on the root height above the lower foot site, no upper bound)
_WALK_WEIGHTS = (0.225, 0.225, 0.050, 0.050, 0.150, 0.150, 0.050, 0.050, 0.025, 0.025)
DEFAULT_REWARD_WEIGHTS = {TASK_JVRC_WALK: _WALK_WEIGHTS, TASK_H1_WALK: _WALK_WEIGHTS, TASK_H1_STAND: (0.3, 0.3, 0.1, 0.1, 0.1, 0.1),
                          TASK_JVRC_STEP: (0.150, 0.150, 0.050, 0.050, 0.450, 0.050)}
DEFAULT_TERMINATION = {TASK_JVRC_WALK: (0.6, 1.4), TASK_H1_WALK: (0.6, 1.4), TASK_H1_STAND: (0.9, 1.4), TASK_JVRC_STEP: (0.6, float("inf"))}


def shaping_weights(task, reward_weights, current):
    """Term weights in REWARD_TERMS[task] order from `reward_weights` -- a dict by term name (partial: the other terms keep `current`) or a
    full sequence.  An unknown name raises KeyError naming the valid ones."""
    names = REWARD_TERMS[task]
    if isinstance(reward_weights, dict):
        unknown = [k for k in reward_weights if k not in names]
        if unknown:
            raise KeyError(f"unknown reward terms {sorted(unknown)}: this task's terms are {list(names)}")
        w = [float(reward_weights.get(k, c)) for k, c in zip(names, current)]
    else:
        w = [float(x) for x in reward_weights]
        if len(w) != len(names):
            raise ValueError(f"{len(w)} reward weights for the {len(names)} terms {list(names)}")
    return np.array(w, dtype=np.float64)


def env_config(task, n_envs, *, frame_skip, kp, kd, seed=0, device=0, max_traj_len=0, env_id_base=0, action_smoothing=1.0,
               nominal_qpos=None, action_offset=None, task_params=None, task_iparams=None, clock_lut=None, init_noise=0.0,
               perturbation=None):
    """(LhwEnvConfig, keep): the struct lhw_env_create reads, and the arrays its pointers refer to (the caller holds `keep` until
    lhw_env_create has returned).  The one place that says what the kernels are told about an env; needs no GPU."""
    keep = []

    def arr(x, dt):
        if x is None:
            return None, 0
        a = np.ascontiguousarray(x, dtype=dt)
        keep.append(a)
        return a.ctypes.data, a.size

    cfg = LhwEnvConfig()
    cfg.task, cfg.n_envs, cfg.device = int(task), int(n_envs), int(device)
    cfg.frame_skip, cfg.max_traj_len, cfg.env_id_base = int(frame_skip), int(max_traj_len), int(env_id_base)
    cfg.seed, cfg.action_smoothing = int(seed) & (2**64 - 1), float(action_smoothing)
    cfg.kp, _ = arr(np.atleast_1d(kp), np.float64)
    cfg.kd, _ = arr(np.atleast_1d(kd), np.float64)
    cfg.nominal_qpos, _ = arr(nominal_qpos, np.float64)
    cfg.action_offset, _ = arr(action_offset, np.float64)
    cfg.task_params, cfg.n_task_params = arr(task_params, np.float64)
    cfg.task_iparams, cfg.n_task_iparams = arr(task_iparams, np.int32)
    cfg.clock_lut, _ = arr(clock_lut, np.float64)
    cfg.period = 0 if clock_lut is None else int(np.asarray(clock_lut).shape[-1])
    cfg.init_noise = float(init_noise)      # radians (base_humanoid_env.py:287: cfg.init_noise degrees * pi / 180)
    if perturbation:                        # JVRC tasks: dict(interval=<control steps>, bodies=[ids], force=, torque=)
        bodies = [int(b) for b in perturbation.get("bodies", [])]
        if len(bodies) > 2:
            raise ValueError("perturbation: at most two bodies")
        cfg.perturb_interval, cfg.n_perturb_bodies = int(perturbation["interval"]), len(bodies)
        for i, b in enumerate(bodies):
            cfg.perturb_bodies[i] = b
        cfg.perturb_force, cfg.perturb_torque = float(perturbation.get("force", 0.0)), float(perturbation.get("torque", 0.0))
    return cfg, keep


class LhwActuatorRand(ctypes.Structure):      # include/lhw.h: lhw_env_set_actuator_randomization / lhw_env_get_actuator_randomization
    _fields_ = [("pdrand_k", ctypes.c_double), ("sim_bemf", ctypes.c_int32), ("bemf_interval", ctypes.c_int32),
                ("bemf_lo", ctypes.c_double), ("bemf_hi", ctypes.c_double)]


# The actuator randomisation an env starts with (lhw_env_get_actuator_randomization on a fresh env; robots/robot_base.py:5, 53-54), in the
# keywords of BatchedEnv.set_actuator_randomization -- which are also the sub-keys of `actuator_randomization:` in an env's YAML
DEFAULT_ACTUATOR_RANDOMIZATION = dict(pdrand_k=0.0, sim_bemf=False, bemf_range=(5.0, 40.0), bemf_interval=10)


class LhwTaskCommands(ctypes.Structure):      # include/lhw.h: lhw_env_set_task_commands / lhw_env_get_task_commands
    _fields_ = [("mode_cdf", ctypes.c_double * 2), ("inplace_yaw", ctypes.c_double * 2), ("forward_vx", ctypes.c_double * 2),
                ("forward_vy", ctypes.c_double * 2), ("switch_stand_every", ctypes.c_int32), ("switch_walk_every", ctypes.c_int32),
                ("step_mode_cdf", ctypes.c_double * 4), ("step_height_start", ctypes.c_double), ("step_height_span", ctypes.c_double),
                ("step_height_max", ctypes.c_double)]


# The task commands an env starts with (lhw_env_get_task_commands on a fresh env: the literals of the reference's tasks/walking_task.py:149-170,
# 194-205 and tasks/stepping_task.py:261-334), by the struct's field names -- the keywords of BatchedEnv.set_task_commands.  The cdfs are
# CUMULATIVE thresholds of the reset draw: STANDING | INPLACE | FORWARD, and CURVED | STANDING | BACKWARD | LATERAL | FORWARD
DEFAULT_TASK_COMMANDS = dict(mode_cdf=(0.6, 0.8), inplace_yaw=(-0.5, 0.5), forward_vx=(0.0, 0.4), forward_vy=(0.0, 0.0), switch_stand_every=100,
                             switch_walk_every=200, step_mode_cdf=(0.15, 0.2, 0.4, 0.7), step_height_start=3000.0, step_height_span=8000.0,
                             step_height_max=0.1)
COMMAND_MODES = ("standing", "inplace", "forward")      # a walking task's mode index (LHW_TIN_MODE, lhw_env_pin_commands) by name
STEP_COMMAND_MODES = ("curved", "standing", "backward", "lateral", "forward")      # the stepping task's, in the order of step_mode_cdf


STEP_MAX_SEQ = 20      # include/lhw.h LHW_STEP_MAX_SEQ: the longest footstep plan


class LhwStepPin(ctypes.Structure):      # include/lhw.h: lhw_env_pin_step_plans / lhw_env_get_pinned_step_plans (one env's pinned footstep plan)
    _fields_ = [("mode", ctypes.c_int32), ("choice", ctypes.c_int32), ("nseq", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("height", ctypes.c_double), ("steps", (ctypes.c_double * 4) * STEP_MAX_SEQ)]


# the same record as a numpy dtype: an array of it is the [count] / [N] argument of the two calls
STEP_PIN_DTYPE = np.dtype([("mode", np.int32), ("choice", np.int32), ("nseq", np.int32), ("reserved", np.int32), ("height", np.float64),
                           ("steps", np.float64, (STEP_MAX_SEQ, 4))])
assert STEP_PIN_DTYPE.itemsize == ctypes.sizeof(LhwStepPin)


def task_commands_struct(fields: dict) -> "LhwTaskCommands":
    """LhwTaskCommands from a full dict by field name (sequences for the array fields)"""
    c = LhwTaskCommands()
    for name, ctype in LhwTaskCommands._fields_:
        v = fields[name]
        if isinstance(getattr(c, name), ctypes.Array):
            v = [float(x) for x in v]
            if len(v) != len(getattr(c, name)):
                raise ValueError(f"task commands: {name} takes {len(getattr(c, name))} values, got {len(v)}")
            setattr(c, name, ctype(*v))
        elif ctype is ctypes.c_int32:
            if int(v) != v:
                raise ValueError(f"task commands: {name} must be an integer, got {v!r}")
            setattr(c, name, int(v))
        else:
            setattr(c, name, float(v))
    return c


def task_commands_dict(c: "LhwTaskCommands") -> dict:
    """the struct as a dict by field name (tuples for the array fields)"""
    return {name: (tuple(getattr(c, name)) if isinstance(getattr(c, name), ctypes.Array) else getattr(c, name)) for name, _ in LhwTaskCommands._fields_}


def cdf_from_probs(probs, names, what="mode_probs"):
    """cumulative thresholds (all but the last, which is 1) of probabilities by `names`; they must sum to 1 within 1e-9"""
    p = [float(probs[k]) for k in names]
    if not all(np.isfinite(p)) or min(p) < 0 or abs(sum(p) - 1.0) > 1e-9:
        raise ValueError(f"{what} {dict(zip(names, p))} must be non-negative and sum to 1")
    return tuple(min(1.0, float(x)) for x in np.cumsum(p)[:-1])


class LhwPpoConfig(ctypes.Structure):      # include/lhw.h: hyper-parameters and shapes of a PPO / LSTM handle
    _fields_ = [
        ("device", ctypes.c_int32), ("obs_dim", ctypes.c_int32), ("act_dim", ctypes.c_int32), ("hidden", ctypes.c_int32),
        ("learn_std", ctypes.c_int32), ("max_rows", ctypes.c_int32), ("lr", ctypes.c_float), ("eps", ctypes.c_float),
        ("clip", ctypes.c_float), ("entropy_coeff", ctypes.c_float), ("mirror_coeff", ctypes.c_float),
        ("max_grad_norm", ctypes.c_float), ("mirror_obs_src", ctypes.c_void_p), ("mirror_obs_sign", ctypes.c_void_p),
        ("mirror_act_src", ctypes.c_void_p), ("mirror_act_sign", ctypes.c_void_p),
    ]


class LhwRolloutPolicy(ctypes.Structure):      # include/lhw.h: the frozen actor as lhw_env_rollout reads it
    _fields_ = [(n, ctypes.c_void_p) for n in ("w1t", "b1", "w2t", "b2", "w3t", "b3", "stdv", "obs_mean", "obs_std")] + [
        (n, ctypes.c_int32) for n in ("obs_dim", "obs_pad", "act_dim", "act_pad", "hidden", "deterministic", "fp16_operands")] + [
        ("seed", ctypes.c_uint64), ("counter", ctypes.c_uint32)]


class LhwTrainStripArgs(ctypes.Structure):      # include/lhw.h: arguments of the test hook lhw_debug_mlp_train_strip
    _fields_ = ([(n, ctypes.c_int32) for n in ("H", "Dp", "O", "Op")] + [(n, ctypes.c_void_p) for n in ("w1", "b1", "w2", "b2", "w3", "b3", "x")] +
                [(n, ctypes.c_int32) for n in ("ldx", "B", "twin0", "critic")] + [(n, ctypes.c_void_p) for n in ("act", "old_logp", "adv", "ret", "stdv")] +
                [("clip", ctypes.c_float), ("mirror_coeff", ctypes.c_float), ("act_src", ctypes.c_void_p), ("act_sign", ctypes.c_void_p)] +
                [(n, ctypes.c_void_p) for n in ("h1", "h2", "y", "dy", "dh2", "dh1", "dstd", "stat_rows")] +
                [("stat_ld", ctypes.c_int32), ("wt_scratch", ctypes.c_void_p)])


class LhwLstmSeqArgs(ctypes.Structure):      # include/lhw.h: arguments of the test hook lhw_debug_lstm_seq
    _fields_ = ([(n, ctypes.c_int32) for n in ("H", "Dp", "T", "Bt", "passes")] +
                [(n, ctypes.c_void_p) for n in ("w1", "bi1", "bh1", "w2", "bi2", "bh2", "reset", "dh2", "xh1", "xh2", "g1", "g2", "c1", "c2", "h2", "scratch")])


class LhwLstmValuesArgs(ctypes.Structure):      # include/lhw.h: arguments of the test hook lhw_debug_lstm_values
    _fields_ = ([(n, ctypes.c_int32) for n in ("H", "D", "Dp", "T", "N")] +
                [(n, ctypes.c_void_p) for n in ("w1", "bi1", "bh1", "w2", "bi2", "bh2", "wo", "bo", "obs_mean", "obs_std", "obs", "term_obs", "done", "reset0",
                                                "xh1", "xh2", "c1", "c2", "val", "vterm", "vfinal", "scratch")])


class LhwRolloutLstmPolicy(ctypes.Structure):      # include/lhw.h: the frozen LSTM actor as lhw_env_rollout_lstm reads it
    _fields_ = [(n, ctypes.c_void_p) for n in ("w1t", "bi1", "bh1", "w2t", "bi2", "bh2", "wot", "bo", "stdv", "obs_mean", "obs_std",
                                               "h1", "h2", "c1", "c2")] + [
        (n, ctypes.c_int32) for n in ("h1_ld", "h2_ld", "state_rows", "obs_dim", "obs_pad", "act_dim", "act_pad", "hidden", "deterministic")] + [
        ("seed", ctypes.c_uint64), ("counter", ctypes.c_uint32)]


class LhwRenderSettings(ctypes.Structure):      # include/lhw.h: lhw_render_frames
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("fovy_deg", ctypes.c_float), ("light_dir", ctypes.c_float * 3),
                ("ambient", ctypes.c_float), ("diffuse", ctypes.c_float), ("background", ctypes.c_float * 3), ("checker_size", ctypes.c_float),
                ("shadows", ctypes.c_int32), ("cull", ctypes.c_int32)]


class LhwJpegSettings(ctypes.Structure):      # include/lhw.h: lhw_jpeg_encode
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("qtable", (ctypes.c_uint16 * 64) * 2)]


RENDER_MAX_GEOMS = 64      # include/lhw.h LHW_RENDER_MAX_GEOMS
RENDER_SCENE_MAX_GEOMS, RENDER_MAX_LAYERS, RENDER_CONE = 256, 8, 32      # include/lhw.h LHW_RENDER_SCENE_MAX_GEOMS / _MAX_LAYERS / _CONE

# include/lhw.h: enum LhwTaskInput (offsets into one env's record, length)
TASK_INPUT_DIM = 176
TASK_INPUT_FIELDS = dict(grf_r=(0, 1), grf_l=(1, 1), contact_z=(2, 1), foot_contact=(3, 1), self_collision=(4, 1), phase=(5, 1), mode=(6, 1),
                         mode_ref=(7, 3), rfoot_vel=(10, 3), lfoot_vel=(13, 3), root_vel_local=(16, 3), root_xpos=(19, 3), head_xpos=(22, 3),
                         rfoot_xpos=(25, 3), lfoot_xpos=(28, 3), qpos=(32, 19), qvel=(51, 18), qacc=(69, 18), act_pos=(87, 12), act_vel=(99, 12),
                         act_tau=(111, 12), prev_torque=(123, 12), prev_action=(135, 12), action=(147, 12), root_xmat=(160, 9))


# include/lhw.h: enum LhwStepTaskInput (the stepping task's second record; offsets into one env's record, length)
STEP_TASK_INPUT_DIM = 32
ROLLOUT_HISTORY_MAX_OBS_PAD = 1024     # include/lhw.h LHW_ROLLOUT_HISTORY_MAX_OBS_PAD: widest padded row lhw_env_rollout_history's in-wave policy step takes
STEP_TASK_INPUT_FIELDS = dict(rsite_xpos=(0, 3), lsite_xpos=(3, 3), target1=(6, 4), target2=(10, 4), reached=(14, 1), frames=(15, 1), t1=(16, 1),
                              t2=(17, 1), nseq=(18, 1), goal=(19, 8), root_xquat=(27, 4))


def split_step_task_inputs(rec):
    """[N][STEP_TASK_INPUT_DIM] records -> dict of named arrays."""
    return {k: (rec[:, o] if n == 1 else rec[:, o:o + n]) for k, (o, n) in STEP_TASK_INPUT_FIELDS.items()}


def split_task_inputs(rec, nq, nv, nu):
    """[N][TASK_INPUT_DIM] records -> dict of named arrays (vectors cut to the model's nq / nv / nu)."""
    cut = dict(qpos=nq, qvel=nv, qacc=nv, act_pos=nu, act_vel=nu, act_tau=nu, prev_torque=nu, prev_action=nu, action=nu)
    out = {}
    for k, (o, n) in TASK_INPUT_FIELDS.items():
        n = cut.get(k, n)
        out[k] = rec[:, o] if n == 1 else rec[:, o:o + n]
    return out


def sources():
    return sorted(glob.glob(os.path.join(_HERE, "csrc", "*.hip")))


# Per-source compile flags of the stepper's translation units.
# -disable-machine-licm: LLVM's machine LICM hoists the materialisation of 64-bit constants (1.0, polynomial coefficients) and of
# lane-derived addresses out of the 25-sub-step loop, the register allocator then parks them in scratch and every use becomes a
# scratch reload (one slot holding the constant 1.0 was reloaded 42 times in the round-3 ISA).  Without it: scratch 480 -> 352 B
# per lane, SGPR spills 438 -> 206, VGPR spills 154 -> 100, control step -5 %.
# -ffp-contract=on (round 5): hipcc's default, fast, lets the BACKEND fuse a multiply with an add wherever the two end up in one
# basic block with the right use counts -- a decision that depends on the code around them, so the same control_step source
# compiled into two kernels (the launch-per-step kernel and the resident rollout kernel) rounded a handful of box-contact
# expressions differently and the two rollouts differed by 1e-15 in the state after a reset.  With `on` the FRONT END fuses, within a
# source expression only: the same source gives the same arithmetic in every kernel (measured: same speed, both kernels bitwise
# equal on all four humanoid tasks).  The GEMM / strip / cartpole kernels keep the default pipeline.
_STEPPER_FLAGS = ["-mllvm", "-disable-machine-licm", "-ffp-contract=on"]
# -amdgpu-sched-strategy=iterative-ilp (round 6, the stepping task's rollout kernels only -- a translation unit of their own): one env per
# wave leaves a third of the lanes idle and the instruction stream latency-bound; LLVM's iterative ILP scheduler makes jvrc_step's rollout
# 3 % faster than the default strategy (max-ilp: 1 %, iterative-maxocc: 2 %, iterative-minreg: 4 % slower).  The two-envs-per-wave kernels
# lose 2.6 % under max-ilp, and this ROCm's clang crashes on their translation unit under iterative-ilp, so they do not get it (they
# take iterative-maxocc, next paragraph); with machine LICM back on the stepping kernels lose 50 % (profiles/r06_stepper_compiler_flags.txt).
# -amdgpu-sched-strategy=iterative-maxocc (round 6, the other stepper translation units): LLVM's iterative scheduler aiming at the kernel's
# occupancy target -- the same 254 VGPRs and no spills, jvrc_walk's rollout 1.8 % faster than under the default strategy.
_MAXOCC = ["-mllvm", "-amdgpu-sched-strategy=iterative-maxocc"]
EXTRA_FLAGS = {"lhw_humanoid.hip": _STEPPER_FLAGS + _MAXOCC, "lhw_humanoid_rollout.hip": _STEPPER_FLAGS + _MAXOCC,
               "lhw_humanoid_rollout_step.hip": _STEPPER_FLAGS + ["-mllvm", "-amdgpu-sched-strategy=iterative-ilp"]}


def _stale(deps) -> bool:
    return not os.path.exists(LIB_PATH) or any(os.path.getmtime(LIB_PATH) < os.path.getmtime(d) for d in deps)


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile liblhw.so for gfx950 in-tree (hipcc cross-compiles without a GPU): one object per source, in parallel, then link.
    Safe under concurrent callers (the ranks of a torch.distributed.run job that all find the library stale): an exclusive file lock
    serialises them and the staleness test is repeated once the lock is held; objects and the library are written under per-process
    temporary names and renamed into place, so nobody can dlopen a half-written file."""
    import fcntl
    srcs = sources()
    deps = srcs + glob.glob(os.path.join(_HERE, "csrc", "*.h")) + glob.glob(os.path.join(_ROOT, "include", "*.h")) + [os.path.abspath(__file__)]
    if not force and not _stale(deps):
        return LIB_PATH
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objdir = os.path.join(_HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    with open(os.path.join(objdir, ".lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not force and not _stale(deps):      # another process built it while this one waited
            return LIB_PATH
        base = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]
        tag = f".{os.getpid()}.tmp"
        procs, objs, tmps = [], [], []
        try:
            for s in srcs:
                o = os.path.join(objdir, os.path.basename(s) + ".o")
                objs.append(o)
                tmps.append(o + tag)
                cmd = base + EXTRA_FLAGS.get(os.path.basename(s), []) + ["-c", s, "-o", o + tag]
                if verbose:
                    print(" ".join(cmd))
                procs.append((cmd, subprocess.Popen(cmd)))
            failed = None
            for cmd, p in procs:
                if p.wait() != 0 and failed is None:
                    failed = (p.returncode, cmd)
                    for _, q in procs:          # one source failed: stop the others instead of leaving them running
                        if q.poll() is None:
                            q.terminate()
            if failed:
                raise subprocess.CalledProcessError(*failed)
            for o in objs:
                os.replace(o + tag, o)
            cmd = base + ["-shared", "-o", LIB_PATH + tag] + objs
            tmps.append(LIB_PATH + tag)
            if verbose:
                print(" ".join(cmd))
            subprocess.check_call(cmd)
            os.replace(LIB_PATH + tag, LIB_PATH)
        finally:
            for _, q in procs:
                if q.poll() is None:
                    q.kill()
                q.wait()
            for t in tmps:
                if os.path.exists(t):
                    os.remove(t)
    return LIB_PATH


def declare(L):
    """Attach the argument types of include/lhw.h's entry points to a loaded library (entry points the library
    does not export are skipped: the emulated test build has no PPO kernels)."""
    vp, i32, i64, u32, u64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_float

    def sig(name, argtypes=None, restype=None):
        f = getattr(L, name, None)
        if f is None:
            return
        if argtypes is not None:
            f.argtypes = argtypes
        if restype is not None:
            f.restype = restype

    sig("lhw_version", restype=ctypes.c_int)
    sig("lhw_last_error", restype=ctypes.c_char_p)
    sig("lhw_env_create", [vp, i64, vp, i64, ctypes.POINTER(LhwEnvConfig), ctypes.POINTER(vp)])
    sig("lhw_env_destroy", [vp])
    for f in ("lhw_env_obs_dim", "lhw_env_act_dim", "lhw_env_num_reward_terms", "lhw_env_nq", "lhw_env_nv"):
        sig(f, [vp])
    sig("lhw_env_reset", [vp, vp, vp, vp])
    sig("lhw_env_step", [vp, vp, vp, vp, vp, vp, vp, vp])
    sig("lhw_env_get_state", [vp, vp, vp])
    sig("lhw_env_set_state", [vp, vp, vp])
    sig("lhw_env_pop_episode_stats", [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(i64)])
    sig("lhw_env_enable_term_stats", [vp, i32])
    sig("lhw_env_pop_term_stats", [vp, vp, ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(i64)])
    sig("lhw_env_set_task_shaping", [vp, vp, i32, vp, i32])
    sig("lhw_env_get_task_shaping", [vp, vp, vp])
    sig("lhw_env_set_actuator_randomization", [vp, ctypes.POINTER(LhwActuatorRand)])
    sig("lhw_env_get_actuator_randomization", [vp, ctypes.POINTER(LhwActuatorRand)])
    sig("lhw_env_get_bemf_damping", [vp, vp])
    sig("lhw_env_set_task_commands", [vp, ctypes.POINTER(LhwTaskCommands)])
    sig("lhw_env_get_task_commands", [vp, ctypes.POINTER(LhwTaskCommands)])
    sig("lhw_env_pin_commands", [vp, i32, i32, vp, vp])
    sig("lhw_env_get_pinned_commands", [vp, vp, vp])
    sig("lhw_env_pin_step_plans", [vp, i32, i32, vp])
    sig("lhw_env_get_pinned_step_plans", [vp, vp])
    sig("lhw_env_set_iteration", [vp, i64])
    sig("lhw_env_pop_fault_stats", [vp, ctypes.POINTER(i64), ctypes.POINTER(i64)])
    sig("lhw_env_pop_rerun_count", [vp, ctypes.POINTER(i64)])
    sig("lhw_env_get_actuator_state", [vp, vp, vp, vp])
    sig("lhw_env_enable_task_inputs", [vp, i32])
    sig("lhw_env_get_task_inputs", [vp, vp])
    sig("lhw_env_task_inputs_device", [vp, ctypes.POINTER(vp)])
    sig("lhw_env_enable_step_task_inputs", [vp, i32])
    sig("lhw_env_get_step_task_inputs", [vp, vp])
    sig("lhw_env_step_task_inputs_device", [vp, ctypes.POINTER(vp)])
    sig("lhw_env_debug_wave_cycles", [vp, vp])
    sig("lhw_debug_gemm", [i32, i32, i32, i32, i32, i32, vp, i32, vp, i32, vp, i32, vp, i32, vp, i32, i32, vp, vp, vp, vp])
    sig("lhw_debug_mlp_strip_forward", [i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp])
    sig("lhw_debug_mlp_strip_backward", [i32, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp])
    sig("lhw_debug_mlp_strip_forward_bits", [i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp])
    sig("lhw_debug_mlp_strip_backward_bits", [i32, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp])
    sig("lhw_debug_mlp_train_strip", [ctypes.POINTER(LhwTrainStripArgs), i32, vp])
    sig("lhw_ppo_debug_set_strip_fused", [vp, i32])
    sig("lhw_ppo_debug_set_strip_wide", [vp, i32])
    sig("lhw_ppo_debug_set_strip_fp16", [vp, i32])
    sig("lhw_debug_mlp_strip_forward_h", [i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp])
    sig("lhw_debug_mlp_strip_backward_h", [i32, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp])
    sig("lhw_ppo_debug_last_grad_fused", [vp])
    sig("lhw_ppo_debug_plan", [vp, i32, i32, ctypes.POINTER(i32)])
    sig("lhw_debug_wgrad_wide", [vp, vp, i32, i32, vp, vp, vp])
    sig("lhw_debug_wgrad_skinny", [i32, i32, i32, i32, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp])
    sig("lhw_debug_dpp_forms", [u64, vp, vp, vp, vp])
    sig("lhw_debug_fastmath", [i64, vp, vp, vp, vp, vp, vp, vp])
    sig("lhw_env_phase_cycles", [vp, ctypes.c_int, vp])
    sig("lhw_env_step_range", [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp])
    sig("lhw_ppo_create", [ctypes.POINTER(LhwPpoConfig), ctypes.POINTER(vp)])
    sig("lhw_ppo_destroy", [vp])
    sig("lhw_ppo_param_count", [vp], i64)
    sig("lhw_ppo_layout", [vp, ctypes.POINTER(i64)])
    sig("lhw_ppo_normalize", [vp, vp, i64, vp, vp, vp, vp, vp])
    sig("lhw_ppo_forward", [vp, vp, vp, i64, vp, vp, u64, u32, u32, ctypes.c_int, vp, vp, vp, vp, vp])
    sig("lhw_ppo_forward_at", [vp, vp, vp, i64, vp, vp, u64, u32, u32, ctypes.c_int, i64, vp, vp, vp, vp, vp])
    sig("lhw_ppo_begin_rollout", [vp, vp, vp])
    sig("lhw_ppo_end_rollout", [vp])
    sig("lhw_ppo_set_inference_dtype", [vp, ctypes.c_int])
    sig("lhw_ppo_set_update_dtype", [vp, ctypes.c_int])
    sig("lhw_ppo_set_imitation", [vp, vp, vp, f32, i64])
    sig("lhw_ppo_grad", [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp])
    sig("lhw_ppo_apply", [vp, vp, vp, vp, vp, i64, f32, vp])
    sig("lhw_ppo_step", [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, i64, f32, vp])
    sig("lhw_ppo_debug_grad_sqnorms", [vp, ctypes.POINTER(f32)])
    sig("lhw_gae", [i32, i32, vp, vp, vp, vp, vp, ctypes.c_double, ctypes.c_double, vp, vp, vp])
    sig("lhw_moments", [vp, i64, vp, vp])
    sig("lhw_scale_shift", [vp, i64, f32, f32, vp])
    sig("lhw_standardize", [vp, i64, vp, ctypes.c_double, vp])
    sig("lhw_rnn_create", [ctypes.POINTER(LhwPpoConfig), i32, i32, i32, ctypes.POINTER(vp)])
    sig("lhw_rnn_destroy", [vp])
    sig("lhw_rnn_param_count", [vp], i64)
    sig("lhw_rnn_layout", [vp, ctypes.POINTER(i64)])
    sig("lhw_rnn_normalize", [vp, vp, i64, vp, vp, vp, vp, vp])
    sig("lhw_rnn_forward", [vp, vp, vp, i64, vp, vp, vp, u64, u32, u32, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, vp])
    sig("lhw_rnn_grad", [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp])
    sig("lhw_rnn_apply", [vp, vp, vp, vp, vp, i64, f32, vp])
    sig("lhw_rnn_debug_grad_sqnorms", [vp, ctypes.POINTER(f32)])
    sig("lhw_rnn_debug_set_seq_fused", [vp, i32])
    sig("lhw_rnn_debug_last_grad_fused", [vp])
    sig("lhw_debug_lstm_seq", [ctypes.POINTER(LhwLstmSeqArgs), i32, vp])
    sig("lhw_debug_lstm_values", [ctypes.POINTER(LhwLstmValuesArgs), i32, vp])
    sig("lhw_rnn_values", [vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp])
    sig("lhw_env_debug_step_record", [vp, vp, vp, vp])
    sig("lhw_env_rollout", [vp, ctypes.POINTER(LhwRolloutPolicy), i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp])
    sig("lhw_env_last_rollout_queued", [vp])
    sig("lhw_env_rollout_task_inputs", [vp, ctypes.POINTER(LhwRolloutPolicy), i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp])
    sig("lhw_env_rollout_step_task_inputs", [vp, ctypes.POINTER(LhwRolloutPolicy), i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp])
    sig("lhw_env_rollout_history", [vp, ctypes.POINTER(LhwRolloutPolicy), i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp])
    sig("lhw_ppo_rollout_policy", [vp, vp, vp, vp, u64, u32, ctypes.c_int, ctypes.POINTER(LhwRolloutPolicy)])
    sig("lhw_debug_policy_step", [ctypes.POINTER(LhwRolloutPolicy), vp, i32, u32, u32, vp, vp, vp, vp])
    sig("lhw_rnn_rollout_policy", [vp, vp, vp, vp, u64, u32, ctypes.c_int, ctypes.POINTER(LhwRolloutLstmPolicy), vp])
    sig("lhw_env_rollout_lstm", [vp, ctypes.POINTER(LhwRolloutLstmPolicy), i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp])
    sig("lhw_debug_lstm_policy_step", [ctypes.POINTER(LhwRolloutLstmPolicy), vp, i32, vp, u32, u32, vp, vp, vp, vp])
    sig("lhw_render_frames", [ctypes.POINTER(LhwRenderSettings), i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp])
    sig("lhw_render_scene", [ctypes.POINTER(LhwRenderSettings), i32, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp])
    sig("lhw_jpeg_scratch_bytes", [ctypes.POINTER(LhwJpegSettings), i32], i64)
    sig("lhw_jpeg_out_bytes", [ctypes.POINTER(LhwJpegSettings), i32], i64)
    sig("lhw_jpeg_encode", [ctypes.POINTER(LhwJpegSettings), i32, vp, vp, i64, vp, i64, vp, vp])
    return L


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise LhwError(-5, f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback for the stepper / PPO kernels)")
    L = declare(ctypes.CDLL(LIB_PATH))
    _LIB = L
    return L


_POISON = os.environ.get("LHW_POISON") == "1"


def empty(*shape, dtype, device):
    """torch.empty for the buffers the kernels fill -- NaN-filled under LHW_POISON=1 (debug: together with the library's 0xFF-filled
    allocations and a -DLHW_POISON build, a kernel that reads what nobody wrote shows up as a NaN instead of as a result that
    depends on what the allocator handed out)."""
    import torch
    t = torch.empty(*shape, dtype=dtype, device=device)
    if _POISON:
        t.fill_(float("nan"))
    return t


def check(rc: int, L=None):
    """raise LhwError with the error text of the library that returned `rc` (None: the GPU library)"""
    if rc != 0:
        raise LhwError(rc, (lib() if L is None else L).lhw_last_error().decode(errors="replace"))
