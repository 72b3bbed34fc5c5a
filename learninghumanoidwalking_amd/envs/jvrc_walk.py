"""JVRC-1 walking task: batched factory mirroring reference envs/jvrc/jvrc_walk.py:13-67,
envs/jvrc/jvrc_base.py:20-145 and envs/jvrc/configs/base.yaml.

The robot model is the hand-authored stand-in ``assets/jvrc_standin.xml`` (the real
jvrc_mj_description submodule is absent from the reference checkout);
pass ``xml_path`` to use a real export of reference envs/jvrc/gen_xml.py instead.
"""
from __future__ import annotations

import os
from dataclasses import dataclass

import numpy as np

from .. import mjcf
from .._lib import TASK_JVRC_WALK
from ..model import fit_stepper_limits
from .humanoid import ASSETS as _ASSETS, HumanoidSpec, WalkingTask, phase_clock_lut  # noqa: F401

JVRC_STANDIN_XML = os.path.join(_ASSETS, "jvrc_standin.xml")
JVRC_BASE_YAML = os.path.join(_ASSETS, "jvrc_base.yaml")

LEG_JOINTS = ["R_HIP_P", "R_HIP_R", "R_HIP_Y", "R_KNEE", "R_ANKLE_R", "R_ANKLE_P",
              "L_HIP_P", "L_HIP_R", "L_HIP_Y", "L_KNEE", "L_ANKLE_R", "L_ANKLE_P"]  # gen_xml.py:44-57

# jvrc_base.py:73-110 (29 robot-state entries) + identity on the external obs; mirrored_acts :110
BASE_MIRROR_OBS = [-0.1, 1, -2, 3, -4, 11, -12, -13, 14, -15, 16, 5, -6, -7, 8, -9, 10,
                   23, -24, -25, 26, -27, 28, 17, -18, -19, 20, -21, 22]
MIRROR_ACTS = [6, -7, -8, 9, -10, 11, 0.1, -1, -2, 3, -4, 5]


@dataclass
class JvrcWalkSpec(WalkingTask, HumanoidSpec):
    yaml_path: str = JVRC_BASE_YAML
    xml_path: str = JVRC_STANDIN_XML

    name = "jvrc_walk"
    task_code = TASK_JVRC_WALK
    base_obs_dim = 37
    act_dim = 12
    step_kernel_name = "humanoid_kernel<0, 1, 32>"     # (MODE 0, TASK_WALK)
    leg_joints = LEG_JOINTS
    task_bodies = ("PELVIS_S", "NECK_P_S", "R_ANKLE_P_S", "L_ANKLE_P_S")
    body_budget = 18        # tree bodies the task's kernel holds per env (fit_stepper_limits)

    def _configure(self, c):
        # BaseHumanoidEnv applies these keys to any env that configures them (base_humanoid_env.py:76-92,221-225,247-305) -- but what
        # the reference DOES with them on a JVRC env differs by key (round 6, read off the reference's code):
        #   observation_noise        ignored: only H1BaseEnv._get_robot_state calls _apply_observation_noise (h1_base.py:107-115);
        #                            JvrcBaseEnv._get_robot_state (jvrc_base.py:133-138) never does -> accepted and ignored here too
        #   dynamics_randomization   raises: randomize_dynamics looks up the body "pelvis" (domain_randomization.py:44), which a JVRC
        #                            model does not have (its root is "PELVIS_S", jvrc_base.py:32) -> KeyError in the reference, refused here
        #   init_noise               runs there (base_humanoid_env.py:260-263, 278-305) and here: root z / roll / pitch / joint noise at every
        #                            reset, in every humanoid kernel (the JVRC auto-reset then computes the reset instead of copying a template)
        #   perturbation             runs there (base_humanoid_env.py:86-92, 224-225; domain_randomization.py:10-26) and here: the wrenches live
        #                            in the per-env HBM record (LhwEnvConfig.perturb_*; at most two bodies, as the H1 kernels)
        if self.perturb_interval <= 0:
            self.perturb_bodies = []        # (a block that is switched off names no bodies to the model fit)
        if len(self.perturb_bodies) > 2:
            raise NotImplementedError(f"perturbation of more than two bodies ({self.perturb_bodies}) in {self.yaml_path}")
        v = c.get("dynamics_randomization")
        if isinstance(v, dict) and v.get("enable", v.get("enabled", False)):
            raise NotImplementedError(f"dynamics_randomization is configured in {self.yaml_path}: the reference itself fails on it for a JVRC model "
                                      "(randomize_dynamics needs a body named 'pelvis', envs/common/domain_randomization.py:44)")
        self.kp, self.kd = np.array(c["kp"], dtype=float), np.array(c["kd"], dtype=float)
        self.half_sitting_pose = np.deg2rad(np.array(c["half_sitting_pose"], dtype=float))
        # jvrc_base.py:52-54
        self.nominal_pose = np.concatenate([[0, 0, 0.81], [1, 0, 0, 0], self.half_sitting_pose])
        self._configure_walking_task(c["task"])
        # jvrc_walk.py:43-63
        self.obs_mean = np.concatenate([np.zeros(5), self.half_sitting_pose, np.zeros(12), [0, 0, 0.5, 0.5, 0.5, 0, 0, 0]])
        self.obs_std = np.concatenate([[0.2, 0.2, 1, 1, 1], 0.5 * np.ones(12), 4 * np.ones(12), [1, 1, 1, 1, 1, 0.5, 0.5, 0.5]])

    def _compile(self):
        return mjcf.compile_file(self.xml_path, self.sim_dt)

    def _build_model(self):
        m = self._compile()
        names = [m.jnt_names[j] for j in m.actuator_trnid]
        if names != LEG_JOINTS or m.nq != 19 or m.nv != 18:
            raise ValueError("model does not have the JVRC leg actuator layout (free root + 12 leg hinges)")
        # a real JVRC export keeps ~30 arm / head / finger links welded to the torso after gen_xml.py:84-87 deleted their
        # joints: they are folded into the bodies they move with (exact; the head stays a body, the task reads its position)
        return fit_stepper_limits(m, self.body_budget, keep=("NECK_P_S",) + tuple(self.perturb_bodies))

    def mirror_inds(self):
        ext = [len(BASE_MIRROR_OBS) + i for i in range(self.base_obs_dim - 29)]
        return BASE_MIRROR_OBS + ext, MIRROR_ACTS, ext[0:2]

    def task_params(self):
        return [self.goal_height]

    def task_iparams(self):
        return self.body_ids()

    def env_args(self):
        model, task, kw = super().env_args()      # (the JVRC kernels take init noise and perturbation from the config record itself)
        return model, task, dict(kw, init_noise=np.deg2rad(self.init_noise_deg), perturbation=self.perturbation_config())

    def algorithmic_bytes_per_env_step(self) -> int:
        """Persistent state record read + written once per control step (168 f64 words) plus
        action in, obs / terminal obs / reward / flags / 10 reward terms out (~2.2 KB)."""
        return 2 * 168 * 8 + 12 * 4 + 2 * 37 * 4 + 4 + 1 + 10 * 4

    def algorithmic_flops_per_env_step(self) -> int:
        """~75 kFLOP per sim sub-step x 25."""
        return 75_000 * self.frame_skip
