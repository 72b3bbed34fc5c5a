"""What the humanoid task specs share: the part of reference envs/common/base_humanoid_env.py and robots/robot_base.py that reads
the YAML config, and the one place that says what a spec hands to the kernels (``env_args``).  Nothing here needs a GPU or torch."""
from __future__ import annotations

import os
from dataclasses import dataclass

import numpy as np
import yaml

ASSETS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "assets")


def load_config(path):
    """YAML config with an optional ``inherits: <file in the same directory>`` key (values of the child win)."""
    with open(path) as f:
        cfg = yaml.safe_load(f)
    cfg.pop("timing", None)
    parent = cfg.pop("inherits", None)
    if parent:
        base = load_config(os.path.join(os.path.dirname(os.path.abspath(path)), parent))
        base.update(cfg)
        cfg = base
    return cfg


def phase_clock_lut(swing_duration, stance_duration, strict_relaxer, freq, period):
    """[4][period] table r_frc, r_vel, l_frc, l_vel of the "grounded" gait clocks at integer phases.

    Restates the knot construction of reference tasks/rewards.py:196-300 (create_phase_reward):
    8 knots per cycle (relaxed ends of right swing, first double stance, left swing, second double
    stance), repeated over three cycles, interpolated with scipy's PchipInterpolator exactly as the
    reference does.  The reference only ever evaluates the splines at integer phases, so the table
    is the whole function.
    """
    from scipy.interpolate import PchipInterpolator
    sw, st = swing_duration * freq, stance_duration * freq
    segs = [(0.0, sw), (sw, sw + st), (sw + st, 2 * sw + st), (2 * sw + st, 2 * (sw + st))]
    x = []
    for a, b in segs:
        off = (b - a) * strict_relaxer
        x += [a + off, b - off]
    x = np.array(x)
    last_off = (segs[3][1] - segs[3][0]) * strict_relaxer
    # right foot force clock: -1 in right swing, +1 otherwise; velocity clocks are the negation; left is the mirror
    r_frc = np.array([-1, -1, 1, 1, 1, 1, 1, 1], dtype=float)
    l_frc = np.array([1, 1, 1, 1, -1, -1, 1, 1], dtype=float)
    r_vel = np.array([1, 1, -1, -1, -1, -1, -1, -1], dtype=float)
    l_vel = np.array([-1, -1, -1, -1, 1, 1, -1, -1], dtype=float)
    xs = np.concatenate([x - x[-1] - last_off, x, x + x[-1] + last_off])
    ph = np.arange(int(period))
    return np.stack([PchipInterpolator(xs, np.tile(y, 3))(ph) for y in (r_frc, r_vel, l_frc, l_vel)])


def mirror_table(mirrored, clock_inds=()):
    """(src, sign): a signed permutation of rl/envs/wrappers.py:78-85 as a gather."""
    n = len(mirrored)
    src, sign = np.zeros(n, np.int32), np.zeros(n, np.float32)
    for i, v in enumerate(mirrored):
        j = int(abs(v))
        src[j], sign[j] = i, np.sign(v)
    for c in clock_inds:
        sign[c] = -sign[c]  # sin(arcsin(c) + pi) == -c (wrappers.py:69-74)
    return src, sign


class WalkingTask:
    """Mixin: the ``task:`` block and gait clock of tasks/walking_task.py (jvrc_walk, jvrc_step, h1_walk)."""

    def _configure_walking_task(self, t):
        self.goal_height = float(t["goal_height"])
        self.total_duration, self.swing_duration, self.stance_duration = (
            float(t["total_duration"]), float(t["swing_duration"]), float(t["stance_duration"]))
        self.period = int(np.floor(2 * self.total_duration * (1 / self.control_dt)))  # walking_task.py:204

    def clock_lut(self):
        return phase_clock_lut(self.swing_duration, self.stance_duration, 0.1, 1 / self.control_dt, self.period)


# The class make_batched instantiates.  None: batched_env.BatchedEnv, looked up at call time so that importing a spec needs no torch.
# A module attribute because callers substitute it: a recorder of the constructor arguments.  (Another build of the library -- a host
# emulation of the kernels -- needs no substitute: it is handed to make_batched as `library`.)
BatchedEnv = None


class BatchedFactory:
    """Mixin of every spec (cartpole included): the GPU env of ``env_args()``."""

    def make_batched(self, n_envs, seed=0, device=0, max_traj_len=0, env_id_base=0, library=None):
        """`library`: BatchedEnv's keyword of that name, passed on only when given."""
        cls = BatchedEnv
        if cls is None:
            from ..batched_env import BatchedEnv as cls
        model, task, kw = self.env_args()
        if library is not None:
            kw = dict(kw, library=library)
        env = cls(model, task, n_envs, seed=seed, device=device, max_traj_len=max_traj_len, env_id_base=env_id_base, **kw)
        shaping = self.task_shaping()
        if shaping is not None:      # (only then: a substituted backend without the method serves every config that does not shape the task)
            env.set_task_shaping(reward_weights=shaping[0], termination=shaping[1])
        actuator = self.actuator_randomization()
        if actuator is not None:     # (likewise)
            env.set_actuator_randomization(**actuator)
        commands = self.commands()
        if commands is not None:     # (likewise)
            env.set_task_commands(**commands)
        return env

    def task_shaping(self):
        return None     # (the humanoid specs read it from the YAML)

    def actuator_randomization(self):
        return None     # (likewise)

    def commands(self):
        return None     # (likewise)


@dataclass
class HumanoidSpec(BatchedFactory):
    """One task on one robot, read from a YAML config.  A subclass states the class attributes below and implements
    ``_configure`` (kp, kd, half_sitting_pose, nominal_pose, obs_mean / obs_std of the BASE observation, task fields),
    ``_build_model``, ``task_params`` and ``task_iparams``."""
    yaml_path: str = ""
    xml_path: str = ""
    obs_dim: int | None = None      # derived (base_obs_dim x obs_history_len); a caller's value is only checked

    name = ""
    task_code = -1                  # the kernels' task: which fused task a plugged-in VectorTask replaces
    base_obs_dim = 0                # width of the observation the task's kernel produces
    act_dim = 0
    step_kernel_name = ""           # rocprof name of the control-step kernel
    leg_joints = ()                 # actuated joints, in action order
    task_bodies = ()                # root, upper body, right foot, left foot

    def __post_init__(self):
        if self.obs_dim not in (None, self.base_obs_dim):
            # the base observation is produced by the task's kernel: its width is not a free parameter of the Spec
            raise ValueError(f"{type(self).__name__}: obs_dim is fixed by the task ({self.base_obs_dim}); got obs_dim={self.obs_dim}")
        c = self.cfg = load_config(self.yaml_path)
        self.sim_dt, self.control_dt = float(c["sim_dt"]), float(c["control_dt"])
        self.history_len = int(c.get("obs_history_len", 1))     # base_humanoid_env.py:53,177-197 (BatchedEnv: shifted in-wave by the resident rollout, by torch ops per launched step)
        if self.history_len < 1:
            raise ValueError("obs_history_len must be >= 1")
        self.action_smoothing = float(c["action_smoothing"])
        self.init_noise_deg = float(c.get("init_noise") or 0.0)     # base_humanoid_env.py:260-263, 278-305
        pc = c.get("perturbation") or {}                            # base_humanoid_env.py:86-92; domain_randomization.py:10-26
        self.perturb_interval = int(pc["interval"] / self.control_dt) if pc.get("enable") else 0
        self.perturb_bodies = list(pc.get("bodies", []))
        self.force_magnitude, self.torque_magnitude = float(pc.get("force_magnitude", 0)), float(pc.get("torque_magnitude", 0))
        # task shaping, no reference counterpart in the YAML (there: literals of tasks/*_task.py): `reward_weights: {term: weight}` (partial,
        # by the names of REWARD_TERMS) and `termination: {min_height:, max_height:}`; checked here, applied by make_batched
        self._shaping = self._read_task_shaping(c)
        # actuator randomisation (robots/robot_base.py:5-62: pdrand_k, sim_bemf -- constructor arguments there, which no shipped env passes):
        # `actuator_randomization: {pdrand_k:, sim_bemf:, bemf_range: [lo, hi], bemf_interval:}`; checked here, applied by make_batched
        self._actuator = self._read_actuator_randomization(c)
        # task commands (tasks/walking_task.py:149-170, 194-205, tasks/stepping_task.py:261-334: literals of the command samplers there):
        # `commands: {mode_probs: {standing:, inplace:, forward:}, inplace_yaw_range: [lo, hi], forward_speed_range:, lateral_speed_range:,
        # switch_standing_every:, switch_walking_every:}`; on jvrc_step `commands: {mode_probs: {curved:, standing:, backward:, lateral:,
        # forward:}, stair_height: {start_iteration:, span_iterations:, max:}}`; checked here, applied by make_batched
        self._commands = self._read_commands(c)
        self._model = None
        self._configure(c)
        # jvrc_walk.py:62-63, h1_env.py:54-55: np.tile over the history
        self.obs_dim = self.base_obs_dim * self.history_len
        self.obs_mean, self.obs_std = np.tile(self.obs_mean, self.history_len), np.tile(self.obs_std, self.history_len)

    @property
    def frame_skip(self) -> int:
        if np.around(self.control_dt % self.sim_dt, 6):  # robot_base.py:37-38
            raise Exception("Control dt should be an integer multiple of Simulation dt.")
        return int(self.control_dt / self.sim_dt)

    def model(self):
        if self._model is None:
            self._model = self._build_model()
        return self._model

    def body_ids(self):
        m = self.model()
        return [m.body_id(b) for b in self.task_bodies]

    def action_offset(self):
        m = self.model()
        return np.array([self.nominal_pose[m.jnt_qposadr[m.jnt_id(j)]] for j in self.leg_joints])  # base_humanoid_env.py:238-245

    def perturbation_config(self):
        """BatchedEnv(perturbation=...) for this YAML (None: off): interval in control steps, packed-model body ids, magnitudes"""
        if self.perturb_interval <= 0:
            return None
        m = self.model()
        return dict(interval=self.perturb_interval, bodies=[m.body_id(b) for b in self.perturb_bodies], force=self.force_magnitude, torque=self.torque_magnitude)

    def _read_task_shaping(self, c):
        from .._lib import DEFAULT_REWARD_WEIGHTS, DEFAULT_TERMINATION, TASK_JVRC_STEP, shaping_weights
        rw, term = c.get("reward_weights"), c.get("termination")
        if rw is None and term is None:
            return None
        weights = shaping_weights(self.task_code, dict(rw or {}), DEFAULT_REWARD_WEIGHTS[self.task_code])
        if not np.isfinite(weights).all():
            raise ValueError(f"reward_weights of {self.yaml_path} must be finite: {rw}")
        term = dict(term or {})
        unknown = set(term) - {"min_height", "max_height"}
        if unknown:
            raise KeyError(f"unknown termination keys {sorted(unknown)} in {self.yaml_path}: min_height, max_height")
        if self.task_code == TASK_JVRC_STEP and "max_height" in term:
            raise ValueError(f"termination.max_height in {self.yaml_path}: the stepping task ends an episode on the root height above the "
                             "lower foot only (min_height); it has no upper bound")
        lo, hi = DEFAULT_TERMINATION[self.task_code]
        lo, hi = float(term.get("min_height", lo)), float(term.get("max_height", hi))
        if not lo < hi:      # (NaN fails it too)
            raise ValueError(f"termination of {self.yaml_path}: min_height {lo} must lie below max_height {hi}")
        return weights, (lo, hi)

    def task_shaping(self):
        """None for a YAML with neither `reward_weights:` nor `termination:` (every config of the reference), else
        (term weights [n_terms] float64 in REWARD_TERMS order -- the YAML's over the reference's --, (lo, hi)): what make_batched hands to
        BatchedEnv.set_task_shaping.  Not part of env_args(): the weights are a run-time setting of the env, not of its creation."""
        return self._shaping

    def _read_actuator_randomization(self, c):
        from .._lib import DEFAULT_ACTUATOR_RANDOMIZATION
        ar = c.get("actuator_randomization")
        if ar is None:
            return None
        ar = dict(ar)
        if ar.pop("sim_motor_dyn", False):
            raise NotImplementedError(f"actuator_randomization.sim_motor_dyn in {self.yaml_path}: the learned motor model's per-joint networks are "
                                      "not part of the reference tree; pdrand_k and sim_bemf are implemented")
        unknown = set(ar) - set(DEFAULT_ACTUATOR_RANDOMIZATION)
        if unknown:
            raise KeyError(f"unknown actuator_randomization keys {sorted(unknown)} in {self.yaml_path}: {', '.join(DEFAULT_ACTUATOR_RANDOMIZATION)}")
        out = dict(DEFAULT_ACTUATOR_RANDOMIZATION, **ar)
        lo, hi = (float(x) for x in out["bemf_range"])
        out.update(pdrand_k=float(out["pdrand_k"]), sim_bemf=bool(out["sim_bemf"]), bemf_range=(lo, hi), bemf_interval=int(out["bemf_interval"]))
        if not 0 <= out["pdrand_k"] < 1:      # (NaN fails it too)
            raise ValueError(f"actuator_randomization.pdrand_k of {self.yaml_path} must lie in [0, 1): {out['pdrand_k']}")
        if not (0 <= lo <= hi < float("inf")) or out["bemf_interval"] < 1:
            raise ValueError(f"actuator_randomization of {self.yaml_path}: bemf_range must be 0 <= lo <= hi (finite), bemf_interval >= 1")
        return out

    def actuator_randomization(self):
        """None for a YAML without `actuator_randomization:` (every shipped config), else the keywords make_batched hands to
        BatchedEnv.set_actuator_randomization -- the YAML's over the reference's defaults.  Not part of env_args(): a run-time setting."""
        return self._actuator

    def _read_commands(self, c):
        from .._lib import COMMAND_MODES, STEP_COMMAND_MODES, TASK_H1_WALK, TASK_JVRC_STEP, TASK_JVRC_WALK, cdf_from_probs
        cm = c.get("commands")
        if cm is None:
            return None
        where = f"commands of {self.yaml_path}"
        if self.task_code not in (TASK_JVRC_WALK, TASK_H1_WALK, TASK_JVRC_STEP):
            raise ValueError(f"{where}: the task of {self.name} has no command")
        cm, out = dict(cm), {}
        stepping = self.task_code == TASK_JVRC_STEP
        ranges = {} if stepping else dict(inplace_yaw_range="inplace_yaw", forward_speed_range="forward_vx", lateral_speed_range="forward_vy")
        every = {} if stepping else dict(switch_standing_every="switch_stand_every", switch_walking_every="switch_walk_every")
        known = ["mode_probs", *ranges, *every] + (["stair_height"] if stepping else [])
        unknown = sorted(set(cm) - set(known))
        if unknown:
            raise KeyError(f"unknown keys {unknown} in {where}: {', '.join(known)}")
        if "mode_probs" in cm:
            names = STEP_COMMAND_MODES if stepping else COMMAND_MODES
            probs = dict(cm["mode_probs"])
            if set(probs) != set(names):
                raise KeyError(f"mode_probs in {where} must give exactly {', '.join(names)}: got {sorted(probs)}")
            try:
                out["step_mode_cdf" if stepping else "mode_cdf"] = cdf_from_probs(probs, names, f"mode_probs in {where}")
            except TypeError as e:
                raise ValueError(f"mode_probs in {where}: {e}") from None
        for key, field in ranges.items():
            if key in cm:
                try:
                    lo, hi = (float(x) for x in cm[key])
                except (TypeError, ValueError):
                    raise ValueError(f"{key} in {where} must be [lo, hi]: {cm[key]!r}") from None
                if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi):
                    raise ValueError(f"{key} in {where} must be finite with lo <= hi: {cm[key]!r}")
                out[field] = (lo, hi)
        for key, field in every.items():
            if key in cm:
                n = cm[key]
                if isinstance(n, bool) or not isinstance(n, int) or n < 0:
                    raise ValueError(f"{key} in {where} must be an integer >= 0 (0: never): {n!r}")
                out[field] = n
        if "stair_height" in cm:
            sh = dict(cm["stair_height"])
            names = dict(start_iteration="step_height_start", span_iterations="step_height_span", max="step_height_max")
            unknown = sorted(set(sh) - set(names))
            if unknown:
                raise KeyError(f"unknown stair_height keys {unknown} in {where}: {', '.join(names)}")
            for key, field in names.items():
                if key in sh:
                    v = float(sh[key])
                    if not np.isfinite(v) or (key == "span_iterations" and v <= 0):
                        raise ValueError(f"stair_height.{key} in {where} must be finite{' and > 0' if key == 'span_iterations' else ''}: {sh[key]!r}")
                    out[field] = v
        return out

    def commands(self):
        """None for a YAML without `commands:` (every shipped config), else the keywords make_batched hands to BatchedEnv.set_task_commands:
        the settings the YAML gives (the others keep the reference's values).  Not part of env_args(): a run-time setting."""
        return self._commands

    def clock_lut(self):
        return None     # (a task with a gait clock mixes in WalkingTask)

    def mirror_inds(self):
        return None     # (mirrored_obs, mirrored_acts, clock_inds) of the env, where the reference defines them

    def mirror_tables(self):
        """((obs_src, obs_sign), (act_src, act_sign)), or None for an env without mirror indices (run_experiment.py:127-128 falls
        back to no mirror)."""
        inds = self.mirror_inds()
        if inds is None:
            return None
        if self.history_len > 1:
            # the reference's mirrored_obs lists base_obs_len indices only (jvrc_walk.py, h1_walk.py): its SymmetricEnv cannot
            # mirror a history observation either
            raise NotImplementedError("mirror loss with obs_history_len > 1: the reference defines mirror indices for the base observation only; train with --no-mirror")
        mo, ma, clock = inds
        return mirror_table(mo, clock), mirror_table(ma)

    def env_args(self):
        """(model, task, kwargs): what BatchedEnv is built from, apart from the per-call n_envs / seed / device / max_traj_len /
        env_id_base.  Pure host arithmetic on the config and the compiled model."""
        return self.model(), self.task_code, dict(
            frame_skip=self.frame_skip, kp=self.kp, kd=self.kd, action_smoothing=self.action_smoothing, nominal_qpos=self.nominal_pose,
            action_offset=self.action_offset(), task_params=self.task_params(), task_iparams=self.task_iparams(),
            clock_lut=self.clock_lut(), history_len=self.history_len)
