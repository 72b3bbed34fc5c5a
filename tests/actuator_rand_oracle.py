"""Float64 oracle of the actuator randomisation (lhw_env_set_actuator_randomization, include/lhw.h), TEST INFRASTRUCTURE ONLY: the
oracle envs of oracle/ with the PD loop of their step() restated as the reference's RobotBase._do_simulation has it with pdrand_k and
sim_bemf on (reference robots/robot_base.py:41-62) -- gains drawn once per control step, a back-EMF damping tau_d redrawn with
probability 1 / bemf_interval and applied to the joint velocity in every sub-step, tau_d born 0 with the robot and untouched by reset().

Draws through oracle/rng.py on the STEP stream under the control-step counter this step's task draws use (env_jvrc_walk.py:182,
env_h1.py:173-185): slot 128 + u kp, 144 + u kd, 160 the back-EMF trigger, 161 + u tau_d -- the kernel's slots (lhw_humanoid_dev.h)."""
import numpy as np

from oracle import rng
from oracle.env_h1 import OracleH1Env
from oracle.env_jvrc_walk import OracleJvrcWalkEnv

SLOT_KP, SLOT_KD, SLOT_BEMF, SLOT_TAU_D = 128, 144, 160, 161


def bemf_fires(seed, env_id, counter, interval=10):
    return rng.randint(seed, env_id, rng.STREAM_STEP, counter, SLOT_BEMF, interval) == 0


class _ActuatorRand:
    """Mixin in front of an oracle env: `pd_loop` is step()'s sub-step loop under the settings below."""
    pdrand_k, sim_bemf, bemf_interval, bemf_lo, bemf_hi = 0.0, False, 10, 5.0, 40.0

    def configure(self, pdrand_k=0.0, sim_bemf=False, bemf_range=(5.0, 40.0), bemf_interval=10):
        self.pdrand_k, self.sim_bemf, self.bemf_interval = float(pdrand_k), bool(sim_bemf), int(bemf_interval)
        self.bemf_lo, self.bemf_hi = (float(x) for x in bemf_range)
        if not hasattr(self, "tau_d"):
            self.tau_d = np.zeros(len(self.gear))      # robot_base.py:25: with the robot, not with the episode
        return self

    def pd_loop(self, act, counter):
        sp, sim = self.spec, self.sim
        s, e, nu = self.seed, self.env_id, len(self.gear)
        kp, kd = np.array(sp.kp, dtype=float), np.array(sp.kd, dtype=float)
        if self.pdrand_k:                                                  # robot_base.py:43-47
            k = self.pdrand_k
            kp = np.array([rng.uniform(s, e, rng.STREAM_STEP, counter, SLOT_KP + u, (1 - k) * kp[u], (1 + k) * kp[u]) for u in range(nu)])
            kd = np.array([rng.uniform(s, e, rng.STREAM_STEP, counter, SLOT_KD + u, (1 - k) * kd[u], (1 + k) * kd[u]) for u in range(nu)])
        if self.sim_bemf and bemf_fires(s, e, counter, self.bemf_interval):   # robot_base.py:53-54
            self.tau_d = np.array([rng.uniform(s, e, rng.STREAM_STEP, counter, SLOT_TAU_D + u, self.bemf_lo, self.bemf_hi) for u in range(nu)])
        for _ in range(sp.frame_skip):                                     # robot_base.py:56-62
            w = self._act_vel()
            tau = kp * (act - self._act_pos()) + kd * (0.0 - w) - self.tau_d * w
            sim.ctrl[:] = tau / self.gear
            sim.step()


class ActJvrcWalkOracle(_ActuatorRand, OracleJvrcWalkEnv):
    def step(self, action):      # OracleJvrcWalkEnv.step with the PD loop replaced
        sp = self.spec
        action = np.asarray(action, dtype=np.float32).astype(np.float64)
        targets = sp.action_smoothing * action + (1 - sp.action_smoothing) * self.prev_prediction
        act = targets + self.offset
        if self.prev_action is None:
            self.prev_action = act
        if self.prev_torque is None:
            self.prev_torque = np.asarray(self._act_torque()).copy()
        self.pd_loop(act, self.step_count)
        self._task_step()
        terms = self._calc_reward(self.prev_torque, self.prev_action, act)
        done = self._done()
        self.prev_action = act
        self.prev_torque = np.asarray(self._act_torque()).copy()
        obs = self.get_obs()
        self.prev_prediction = action
        self._post_obs_perturbation()
        self.traj_len += 1
        return obs, sum(terms.values()), done, terms


class ActH1Oracle(_ActuatorRand, OracleH1Env):
    def step(self, action):      # OracleH1Env.step with the PD loop replaced
        sp = self.spec
        action = np.asarray(action, dtype=np.float32).astype(np.float64)
        targets = sp.action_smoothing * action + (1 - sp.action_smoothing) * self.prev_prediction
        act = targets + self.offset
        if self.prev_action is None:
            self.prev_action = act
        if self.prev_torque is None:
            self.prev_torque = np.asarray(self._act_torque()).copy()
        self.pd_loop(act, self.step_count)
        self._task_step(self.step_count)
        terms = self._calc_reward(self.prev_torque, self.prev_action, act)
        done = self._done()
        self.prev_action = act
        self.prev_torque = np.asarray(self._act_torque()).copy()
        obs = self.get_obs()
        self.prev_prediction = action
        c = self.step_count
        if sp.dynrand_interval > 0 and rng.randint(self.seed, self.env_id, rng.STREAM_STEP, c, 0, sp.dynrand_interval) == 0:
            self._randomize_dynamics(rng.STREAM_STEP, c, 1)
        if sp.perturb_interval > 0 and rng.randint(self.seed, self.env_id, rng.STREAM_STEP, c, 70, sp.perturb_interval) == 0:
            self._apply_perturbation(c)
        self.step_count += 1
        self.traj_len += 1
        return obs, sum(terms.values()), done, terms


ORACLES = {"jvrc_walk": ActJvrcWalkOracle, "h1": ActH1Oracle}
