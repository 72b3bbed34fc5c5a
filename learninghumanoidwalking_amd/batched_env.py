"""Batched environments on one MI355X: thin Python host over the C ABI (include/lhw.h).

`BatchedEnv` is what the trainer uses (N envs advanced by one kernel launch per control
step); the N=1 `BaseHumanoidEnv`-shaped adapters live in ``envs/``.  torch is used only to
own device buffers and streams.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import REWARD_TERMS, TASK_CARTPOLE, TASK_H1_STAND, TASK_H1_WALK, TASK_JVRC_STEP, TASK_JVRC_WALK  # noqa: F401
from .model import Model

DONE_TERMINATED, DONE_TRUNCATED = 1, 2


def term_stats_dict(term_sum, terminated: int, truncated: int, names) -> dict:
    """dict(episodes, terminated, truncated, terms={name: mean over the finished episodes of the episode's sum of that term}) from the
    sums lhw_env_pop_term_stats returns (NaN means while no episode has finished)."""
    episodes = int(terminated) + int(truncated)
    mean = [float(s) / episodes if episodes else float("nan") for s in term_sum]
    return dict(episodes=episodes, terminated=int(terminated), truncated=int(truncated), terms=dict(zip(names, mean)))


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream_ptr(device):
    """The current stream of a GPU device; None for a CPU one (a host build of the library, which takes a null stream)."""
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream) if device.type == "cuda" else None


def history_update(prev_full: torch.Tensor, base_obs: torch.Tensor, term_base: torch.Tensor, done: torch.Tensor, base: int):
    """Observation history of the reference (envs/common/base_humanoid_env.py:177-197, 274): the observation is a deque of the
    last `history_len` base observations, newest first, flattened; a reset empties it and zero-fills before the first push.
    prev_full [n, H*base]: the full observation before this control step; base_obs: what the kernel returns (for an env whose
    episode ended: the first observation after the auto-reset); term_base: the base observation of the state the step reached;
    done [n] uint8.  Returns (full observation, full terminal observation), both [n, H*base]."""
    tail = prev_full[:, :-base]
    keep = (done == 0).to(prev_full.dtype).unsqueeze(1)
    return torch.cat([base_obs, tail * keep], dim=1), torch.cat([term_base, tail], dim=1)


class BatchedEnv:
    """N copies of one task, state resident in HBM.

    Mirrors, per env, the reference's ``env.reset()`` / ``env.step(a)`` contract (reference
    envs/common/base_humanoid_env.py:199-276) plus the episode bookkeeping of
    ``RolloutWorker.sample`` (reference rl/workers/rollout_worker.py:142-181) when
    ``max_traj_len > 0``.
    """

    def __init__(self, model: Model, task: int, n_envs: int, *, device: int | torch.device = 0, history_len: int = 1, library=None, **config):
        """`config`: the keywords of _lib.env_config (frame_skip, kp, kd, seed, max_traj_len, env_id_base, action_smoothing, ...).
        `library`: a ctypes handle of another build of the C ABI that _lib.declare was applied to (None: _lib.lib(), the GPU library);
        only with one may `device` be a CPU device -- the buffers are then CPU tensors and the calls get a null stream."""
        if library is None and not torch.cuda.is_available():
            raise _lib.LhwError(-5, "no GPU visible: BatchedEnv has no CPU fallback")
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if library is None and self.device.type != "cuda":
            raise _lib.LhwError(-5, f"device {self.device}: BatchedEnv has no CPU fallback")
        self.model = model
        self.n_envs = int(n_envs)
        self.task = task
        self._ib, self._db = model.pack()
        cfg, _keep = _lib.env_config(task, self.n_envs, device=self.device.index or 0, **config)    # (_keep: until lhw_env_create has copied them)
        self.env_id_base = cfg.env_id_base      # global index of env 0: every RNG key of the kernels uses env_id_base + n
        self._h = ctypes.c_void_p()
        self._L = L = _lib.lib() if library is None else library
        self._check(L.lhw_env_create(self._ib.ctypes.data, self._ib.size, self._db.ctypes.data, self._db.size,
                                    ctypes.byref(cfg), ctypes.byref(self._h)))
        # obs_history_len > 1 (base_humanoid_env.py:177-197): obs_dim is the full length.  The resident rollout shifts the history rows
        # inside the stepper's wavefronts (lhw_env_rollout_history); the launch-per-step calls (step / step_range / reset) get the base
        # observation from the kernels and shift the rows by a few torch ops per step (history_update) -- the same values
        self.base_obs_dim = L.lhw_env_obs_dim(self._h)
        self.history_len = int(history_len)
        if self.history_len < 1:
            raise ValueError("history_len must be >= 1")
        self.obs_dim = self.base_obs_dim * self.history_len
        self.act_dim = L.lhw_env_act_dim(self._h)
        self.n_terms = L.lhw_env_num_reward_terms(self._h)
        self.nq, self.nv = L.lhw_env_nq(self._h), L.lhw_env_nv(self._h)
        N, dev = self.n_envs, self.device
        self.obs = torch.zeros(N, self.obs_dim, dtype=torch.float32, device=dev)
        self.term_obs = torch.zeros(N, self.obs_dim, dtype=torch.float32, device=dev)
        self.rew = torch.zeros(N, dtype=torch.float32, device=dev)
        self.done = torch.zeros(N, dtype=torch.uint8, device=dev)
        self.rew_terms = torch.zeros(N, self.n_terms, dtype=torch.float32, device=dev)
        if self.history_len > 1:
            self._base = torch.zeros(N, self.base_obs_dim, dtype=torch.float32, device=dev)    # kernel outputs
            self._tbase = torch.zeros(N, self.base_obs_dim, dtype=torch.float32, device=dev)
            self._full = torch.zeros(N, self.obs_dim, dtype=torch.float32, device=dev)         # current full observation

    def _check(self, rc: int):
        _lib.check(rc, self._L)     # (the error text of this env's own library)

    def _here(self, *tensors) -> bool:
        """every tensor is on this env's device (the index compared only where both sides carry one: torch.device("cuda") has none)"""
        d = self.device
        return all(t.device.type == d.type and (t.device.index is None or d.index is None or t.device.index == d.index) for t in tensors)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.lhw_env_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, mask: torch.Tensor | None = None, obs_out: torch.Tensor | None = None) -> torch.Tensor:
        """Reset the envs whose mask byte is non-zero (None: all).  The first observation of the reset envs goes to `obs_out`
        ([N, obs_dim], rows of the other envs untouched) or, by default, to self.obs."""
        if mask is not None:
            assert mask.dtype == torch.uint8 and self._here(mask) and mask.numel() == self.n_envs
        if obs_out is None or self.history_len > 1:     # (a history env always resets into its own buffer)
            obs_out = self.obs
        else:
            assert self._here(obs_out) and obs_out.dtype == torch.float32 and obs_out.is_contiguous() and obs_out.shape == self.obs.shape
        self._check(self._L.lhw_env_reset(self._h, _ptr(mask), _ptr(self._kernel_out(obs_out)[0]), _stream_ptr(self.device)))
        if self.history_len > 1:
            sel = slice(None) if mask is None else mask.bool()
            self._full[sel] = 0
            self._full[sel, :self.base_obs_dim] = self._base[sel]
            self.obs.copy_(self._full)
        return obs_out

    def _kernel_out(self, obs, tob=None):
        """The (observation, terminal observation) buffers the kernels write: the caller's, or the base-observation buffers of a
        history env (whose full observations _history then builds)."""
        return (obs, tob) if self.history_len == 1 else (self._base, self._tbase)

    def _history(self, a, b, obs, tob, done):
        """full observation / terminal observation of envs [a, b) from the kernel's base outputs (history envs only)"""
        if self.history_len == 1:
            return
        full, term = history_update(self._full[a:b], self._base[a:b], self._tbase[a:b], done[a:b], self.base_obs_dim)
        self._full[a:b] = full
        obs[a:b] = full
        tob[a:b] = term

    def step(self, act: torch.Tensor, obs_out: torch.Tensor | None = None, term_obs_out: torch.Tensor | None = None,
             rew_out: torch.Tensor | None = None, done_out: torch.Tensor | None = None):
        """act [N, act_dim] float32 on device.  Returns (obs, rew, done, term_obs) device tensors."""
        assert self._here(act) and act.dtype == torch.float32 and act.is_contiguous() and act.numel() == self.n_envs * self.act_dim
        obs = self.obs if obs_out is None else obs_out
        tob = self.term_obs if term_obs_out is None else term_obs_out
        rew = self.rew if rew_out is None else rew_out
        done = self.done if done_out is None else done_out
        kobs, ktob = self._kernel_out(obs, tob)
        self._check(self._L.lhw_env_step(self._h, _ptr(act), _ptr(kobs), _ptr(ktob), _ptr(rew), _ptr(done), _ptr(self.rew_terms),
                                        _stream_ptr(self.device)))
        self._history(0, self.n_envs, obs, tob, done)
        return obs, rew, done, tob

    def step_range(self, first: int, count: int, act: torch.Tensor, obs: torch.Tensor, term_obs: torch.Tensor, rew: torch.Tensor,
                   done: torch.Tensor):
        """Advance envs [first, first + count) only, on the current stream.  All tensors are the FULL-batch buffers ([N, ...]);
        independent groups issued on different streams overlap on the GPU (no batch-wide barrier per control step)."""
        assert self._here(act) and act.dtype == torch.float32 and act.is_contiguous() and act.numel() == self.n_envs * self.act_dim
        kobs, ktob = self._kernel_out(obs, term_obs)
        self._check(self._L.lhw_env_step_range(self._h, int(first), int(count), _ptr(act), _ptr(kobs), _ptr(ktob), _ptr(rew), _ptr(done),
                                              _ptr(self.rew_terms), _stream_ptr(self.device)))
        self._history(int(first), int(first) + int(count), obs, term_obs, done)

    def rollout(self, policy, T: int, obs: torch.Tensor, act: torch.Tensor, logp: torch.Tensor, term_obs: torch.Tensor, rew: torch.Tensor,
                done: torch.Tensor, first: int = 0, count: int | None = None, task_inputs: torch.Tensor | None = None,
                step_task_inputs: torch.Tensor | None = None) -> bool:
        """The resident rollout (lhw_env_rollout): T control steps of envs [first, first + count) in ONE launch on the current
        stream, the actor (`policy`: PpoKernels.rollout_policy()) evaluated inside the stepper's wavefronts -- the body of
        RolloutWorker.sample's loop (reference rl/workers/rollout_worker.py:142-181) with no wavefront waiting for another env.
        Buffers are time-major over the full batch: obs [T + 1, N, D] (slice 0 in), act [T, N, A], logp / rew / done [T, N],
        term_obs [T, N, D].  `task_inputs` [T, N, TASK_INPUT_DIM] float64 (optional): the sim-facade record of EVERY control step
        (lhw_env_rollout_task_inputs), for reward-only task plug-ins; `step_task_inputs` [T, N, STEP_TASK_INPUT_DIM] float64 (stepping
        task only, together with `task_inputs`): the stepping task's second record of every control step as well
        (lhw_env_rollout_step_task_inputs).  An env with an observation history (history_len > 1) goes through
        lhw_env_rollout_history: the wavefronts shift the history rows themselves, obs[0] is the state they start from, and the env's
        own copy of the current full observation is set to obs[T] afterwards, so launch-per-step calls may follow.  Returns False
        (nothing launched) where the library has no resident kernel for this env / policy; a HIP failure raises."""
        if policy is None:
            return False
        L, bufs, head = self._L, (obs, act, logp, term_obs, rew, done), ()
        if self.history_len > 1:
            fn, records, head = L.lhw_env_rollout_history, 2, (self.history_len,)
        elif step_task_inputs is not None:
            fn, records = L.lhw_env_rollout_step_task_inputs, 2
        elif task_inputs is not None:
            fn, records = L.lhw_env_rollout_task_inputs, 1
        else:
            fn, records = L.lhw_env_rollout, 0
        ok = self._resident(fn, policy, T, bufs, first, count, task_inputs, step_task_inputs, records, head=head)
        if ok and self.history_len > 1:      # the launch-per-step calls continue from the rollout's last observation (a device copy behind the launch)
            a, b = int(first), int(first) + (int(self.n_envs - first) if count is None else int(count))
            self._full[a:b].copy_(obs[T, a:b])
        return ok

    def _resident(self, fn, policy, T, bufs, first, count, task_inputs, step_task_inputs, records, head=(), flags=()) -> bool:
        """What the resident-rollout entry points share: the checks of the buffers (obs, act, logp, term_obs, rew, done), of `flags` ([N] uint8
        each) and of the task-input records, the call, and its result: False where the library declines (LHW_ERR_UNSUPPORTED: the caller keeps
        the launch-per-step pipeline), anything else -- LHW_ERR_HIP ... -- raises.  What `fn` takes besides the common arguments: `head`
        (integers) behind T, the flags behind rew_terms, then the first `records` of (task_inputs, step_task_inputs)."""
        N = self.n_envs
        obs, act, logp, term_obs, rew, done = bufs
        assert obs.shape == (T + 1, N, self.obs_dim) and act.shape == (T, N, self.act_dim) and term_obs.shape == (T, N, self.obs_dim)
        assert logp.shape == (T, N) and rew.shape == (T, N) and done.shape == (T, N) and done.dtype == torch.uint8
        for x in flags:
            assert x.shape == (N,) and x.dtype == torch.uint8
        for x in bufs + tuple(flags):
            assert self._here(x) and x.is_contiguous()
        if step_task_inputs is not None:
            assert task_inputs is not None, "the stepping record is exported together with the LhwTaskInput one"
            assert step_task_inputs.shape == (T, N, _lib.STEP_TASK_INPUT_DIM) and step_task_inputs.dtype == torch.float64
            assert self._here(step_task_inputs) and step_task_inputs.is_contiguous()
        if task_inputs is not None:
            assert task_inputs.shape == (T, N, _lib.TASK_INPUT_DIM) and task_inputs.dtype == torch.float64 and self._here(task_inputs) and task_inputs.is_contiguous()
        tail = tuple(flags) + (task_inputs, step_task_inputs)[:records]
        rc = fn(self._h, ctypes.byref(policy), int(first), int(N - first if count is None else count), int(T), *head, *(_ptr(x) for x in bufs),
                _ptr(self.rew_terms), *(_ptr(x) for x in tail), _stream_ptr(self.device))
        if rc == -4:
            return False
        self._check(rc)
        return True

    def rollout_lstm(self, policy, T: int, obs: torch.Tensor, act: torch.Tensor, logp: torch.Tensor, term_obs: torch.Tensor, rew: torch.Tensor,
                     done: torch.Tensor, reset0: torch.Tensor, first: int = 0, count: int | None = None, task_inputs: torch.Tensor | None = None,
                     step_task_inputs: torch.Tensor | None = None) -> bool:
        """The resident rollout for an LSTM actor (lhw_env_rollout_lstm): as `rollout`, with `policy` = RnnKernels.rollout_policy() --
        whose state buffers the launch reads and writes -- and `reset0` [N] uint8: the envs whose episode starts with obs[0] (their state
        counts as zero; afterwards the state is zeroed wherever the previous step's done flag is set: reference
        rl/workers/rollout_worker.py:130-190).  Returns False (nothing launched) where the library has no such kernel for this env / policy."""
        if self.history_len > 1 or policy is None:
            return False
        return self._resident(self._L.lhw_env_rollout_lstm, policy, T, (obs, act, logp, term_obs, rew, done), first, count, task_inputs, step_task_inputs, 2,
                              flags=(reset0,))

    def last_rollout_queued(self) -> bool:
        """the most recent resident rollout drained the job queue (stepping task with more envs than wave slots)"""
        return self._L.lhw_env_last_rollout_queued(self._h) == 1

    def get_state(self):
        qpos = np.zeros((self.n_envs, self.nq))
        qvel = np.zeros((self.n_envs, self.nv))
        self._check(self._L.lhw_env_get_state(self._h, qpos.ctypes.data, qvel.ctypes.data))
        return qpos, qvel

    def set_state(self, qpos, qvel):
        qpos = np.ascontiguousarray(qpos, dtype=np.float64).reshape(self.n_envs, self.nq)
        qvel = np.ascontiguousarray(qvel, dtype=np.float64).reshape(self.n_envs, self.nv)
        self._check(self._L.lhw_env_set_state(self._h, qpos.ctypes.data, qvel.ctypes.data))

    def task_shaping(self):
        """({term name: weight} in the order of rew_terms, (lo, hi)): the reward-term weights and termination bounds this env's kernels
        apply, read back from the library (lhw_env_get_task_shaping; humanoid tasks only)."""
        w, lim = np.zeros(self.n_terms), np.zeros(2)
        self._check(self._L.lhw_env_get_task_shaping(self._h, w.ctypes.data, lim.ctypes.data))
        return dict(zip(REWARD_TERMS[self.task], w.tolist())), (float(lim[0]), float(lim[1]))

    def set_task_shaping(self, reward_weights=None, termination=None):
        """Reward-term weights and / or termination bounds of the fused task, for the whole batch from the next launch on
        (lhw_env_set_task_shaping: synchronises the device; episodes in flight carry on under the new values -- a reward curriculum may
        call this between iterations).  `reward_weights`: a dict by the names of REWARD_TERMS[task] (partial: the other terms keep their
        current weight; an unknown name raises KeyError) or a full sequence in that order.  `termination`: (lo, hi) on the root height
        (stepping task: on the root height above the lower foot site, hi must stay +inf); +-inf switch a bound off."""
        w = lim = None
        if reward_weights is not None:
            w = _lib.shaping_weights(self.task, reward_weights, self.task_shaping()[0].values())
        if termination is not None:
            lim = np.array([float(x) for x in termination], dtype=np.float64)
        self._check(self._L.lhw_env_set_task_shaping(self._h, w.ctypes.data if w is not None else None, 0 if w is None else w.size,
                                                    lim.ctypes.data if lim is not None else None, 0 if lim is None else lim.size))

    @property
    def actuator_randomization(self) -> dict:
        """dict(pdrand_k, sim_bemf, bemf_range, bemf_interval): the actuator randomisation this env's kernels apply, read back from the
        library (lhw_env_get_actuator_randomization; humanoid tasks only) in the keywords of set_actuator_randomization."""
        a = _lib.LhwActuatorRand()
        self._check(self._L.lhw_env_get_actuator_randomization(self._h, ctypes.byref(a)))
        return dict(pdrand_k=a.pdrand_k, sim_bemf=bool(a.sim_bemf), bemf_range=(a.bemf_lo, a.bemf_hi), bemf_interval=int(a.bemf_interval))

    def set_actuator_randomization(self, pdrand_k=0.0, sim_bemf=False, bemf_range=(5.0, 40.0), bemf_interval=10):
        """The two sim-to-real settings of the reference's PD law (robots/robot_base.py:5-62), for the whole batch from the next control
        step on (lhw_env_set_actuator_randomization: synchronises the device).  `pdrand_k` in [0, 1): every control step draws its gains
        per env and actuator from U((1 - k) kp, (1 + k) kp), kd likewise.  `sim_bemf`: with probability 1 / `bemf_interval` a control
        step redraws the env's back-EMF damping tau_d ~ U(*bemf_range), which every sub-step applies to the joint velocity; tau_d
        survives resets and is zeroed by the call that turns sim_bemf off.  Every argument not given takes the reference's value (off).
        While either is on, an LSTM policy or an observation history samples launch per step (their resident rollouts are declined)."""
        lo, hi = (float(x) for x in bemf_range)
        a = _lib.LhwActuatorRand(float(pdrand_k), int(bool(sim_bemf)), int(bemf_interval), lo, hi)
        self._check(self._L.lhw_env_set_actuator_randomization(self._h, ctypes.byref(a)))

    def bemf_damping(self):
        """[N, act_dim] float64: every env's back-EMF damping tau_d (host copy, synchronous; lhw_env_get_bemf_damping)"""
        out = np.zeros((self.n_envs, self.act_dim))
        self._check(self._L.lhw_env_get_bemf_damping(self._h, out.ctypes.data))
        return out

    def get_task_commands(self) -> dict:
        """The settings of the fused task's command sampler this env's kernels apply, read back from the library
        (lhw_env_get_task_commands; jvrc_walk, h1_walk, jvrc_step), by the field names of LhwTaskCommands: _lib.DEFAULT_TASK_COMMANDS on a
        fresh env."""
        c = _lib.LhwTaskCommands()
        self._check(self._L.lhw_env_get_task_commands(self._h, ctypes.byref(c)))
        return _lib.task_commands_dict(c)

    def set_task_commands(self, **fields):
        """Settings of the fused task's command sampler, for the whole batch from the next control step on (lhw_env_set_task_commands:
        synchronises the device).  Keywords are the fields of LhwTaskCommands -- mode_cdf (cumulative: standing | inplace | forward),
        inplace_yaw / forward_vx / forward_vy (lo, hi), switch_stand_every / switch_walk_every (0: never) for the walking tasks;
        step_mode_cdf (curved | standing | backward | lateral | forward), step_height_start / _span / _max for jvrc_step -- and those not
        given keep their current value.  An unknown keyword raises KeyError."""
        unknown = sorted(set(fields) - set(_lib.DEFAULT_TASK_COMMANDS))
        if unknown:
            raise KeyError(f"unknown task command settings {unknown}: {', '.join(_lib.DEFAULT_TASK_COMMANDS)}")
        c = _lib.task_commands_struct(dict(self.get_task_commands(), **fields))
        self._check(self._L.lhw_env_set_task_commands(self._h, ctypes.byref(c)))

    def _env_range(self, envs):
        """(first, count) of `envs`: None (all), an int, or a range / sequence of consecutive env indices"""
        if envs is None:
            return 0, self.n_envs
        idx = [int(envs)] if np.ndim(envs) == 0 else [int(k) for k in envs]
        if idx and idx != list(range(idx[0], idx[0] + len(idx))):
            raise ValueError(f"envs must be consecutive indices, got {idx}")
        return (idx[0], len(idx)) if idx else (0, 0)

    def pin_commands(self, mode, ref, envs=None):
        """Pin the command of `envs` (None: all; an index or consecutive indices) on a walking task: `mode` ("standing" / "inplace" /
        "forward" or 0 / 1 / 2, one for all or one per env; -1 frees) and `ref` = mode_ref {yaw rate, forward speed, lateral speed} ([3] for
        all or [count][3]).  The kernels then use them for those envs instead of drawing, across auto-resets, from the next control step
        on (lhw_env_pin_commands: synchronises the device).  Pin before the reset whose observation a rollout starts from."""
        first, count = self._env_range(envs)
        code = lambda m: _lib.COMMAND_MODES.index(m) if isinstance(m, str) else int(m)      # noqa: E731
        modes = np.array([code(m) for m in mode] if np.ndim(mode) else [code(mode)] * count, dtype=np.int32)
        refs = np.ascontiguousarray(np.broadcast_to(np.asarray(ref, dtype=np.float64), (count, 3)))
        if modes.shape != (count,):
            raise ValueError(f"{modes.size} modes for {count} envs")
        self._check(self._L.lhw_env_pin_commands(self._h, first, count, modes.ctypes.data, refs.ctypes.data))

    def unpin_commands(self, envs=None):
        """Free `envs` (None: all): their commands are drawn again, from the next reset or switch on."""
        first, count = self._env_range(envs)
        self.pin_commands(-1, np.zeros(3), envs=range(first, first + count))

    def pinned_commands(self):
        """(mode [N] int32, -1 for a free env; ref [N][3] float64) of the whole batch (lhw_env_get_pinned_commands)"""
        mode, ref = np.zeros(self.n_envs, np.int32), np.zeros((self.n_envs, 3))
        self._check(self._L.lhw_env_get_pinned_commands(self._h, mode.ctypes.data, ref.ctypes.data))
        return mode, ref

    def pin_step_plans(self, mode, *, height=None, choice=None, steps=None, envs=None):
        """Pin the walk mode and footstep plan of `envs` (None: all; an index or consecutive indices) on jvrc_step, instead of the draws of
        the task reset (lhw_env_pin_step_plans: synchronises the device; acts from each env's next reset on, across auto-resets).
        `mode`: a name of _lib.STEP_COMMAND_MODES or its code, one for all or one per env; -1 frees.  `height` (forward): the signed rise
        per step, instead of the stair schedule and the sign draw; None / NaN: both as drawn.  `choice`: the row of the plan table
        (curved) or 0 / 1 for the side (lateral); None / -1: as drawn.  Both one for all or one per env.  `steps`: an explicit plan of
        2..20 steps [n][4] = x, y, z, theta relative to the feet mid-point and the root yaw at the reset ([n][3] = x, y, theta: z = 0),
        one for all or a list of one per env (None in it: that env's sequence is generated from its mode).  Pin before the reset whose
        observation a rollout starts from."""
        first, count = self._env_range(envs)
        code = lambda m: _lib.STEP_COMMAND_MODES.index(m) if isinstance(m, str) else int(m)      # noqa: E731

        def per_env(v, what, dtype, default):
            if v is None:
                return np.full(count, default, dtype=dtype)
            a = np.array([default if x is None else x for x in v] if np.ndim(v) else [v] * count, dtype=dtype)
            if a.shape != (count,):
                raise ValueError(f"{a.size} values of {what} for {count} envs")
            return a

        pins = np.zeros(count, dtype=_lib.STEP_PIN_DTYPE)
        pins["mode"] = per_env([code(m) for m in mode] if np.ndim(mode) else code(mode), "mode", np.int32, -1)
        pins["choice"] = per_env(choice, "choice", np.int32, -1)
        pins["height"] = per_env(height, "height", np.float64, np.nan)
        if steps is not None:
            one = not isinstance(steps, (list, tuple)) or (len(steps) > 0 and np.ndim(steps[0]) == 1)      # [n][3 | 4]: one plan for all
            plans = [steps] * count if one else list(steps)
            if len(plans) != count:
                raise ValueError(f"{len(plans)} plans for {count} envs")
            for i, plan in enumerate(plans):
                if plan is None:
                    continue
                plan = np.asarray(plan, dtype=np.float64)
                if plan.ndim != 2 or plan.shape[1] not in (3, 4) or not 2 <= plan.shape[0] <= _lib.STEP_MAX_SEQ:
                    raise ValueError(f"a footstep plan is [n][3] (x, y, theta) or [n][4] (x, y, z, theta) with 2 <= n <= {_lib.STEP_MAX_SEQ}: got shape {plan.shape}")
                pins["nseq"][i] = plan.shape[0]
                pins["steps"][i, :plan.shape[0]] = plan if plan.shape[1] == 4 else np.insert(plan, 2, 0.0, axis=1)
        self._check(self._L.lhw_env_pin_step_plans(self._h, first, count, pins.ctypes.data))

    def unpin_step_plans(self, envs=None):
        """Free `envs` (None: all): from their next reset on, mode and plan are drawn again."""
        first, count = self._env_range(envs)
        self.pin_step_plans(-1, envs=range(first, first + count))

    def pinned_step_plans(self):
        """The whole batch's pins as a numpy record array [N] of _lib.STEP_PIN_DTYPE -- mode (-1 for a free env, whose other fields are
        zero), choice, nseq, reserved, height, steps [20][4] (lhw_env_get_pinned_step_plans)"""
        out = np.zeros(self.n_envs, dtype=_lib.STEP_PIN_DTYPE)
        self._check(self._L.lhw_env_get_pinned_step_plans(self._h, out.ctypes.data))
        return out

    def pop_episode_stats(self):
        r, l, c = ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
        self._check(self._L.lhw_env_pop_episode_stats(self._h, ctypes.byref(r), ctypes.byref(l), ctypes.byref(c)))
        return r.value, l.value, c.value

    def enable_term_stats(self, enable: bool = True):
        """Arm / disarm the per-term episode statistics (lhw_env_enable_term_stats): from the next control step on the kernels keep,
        per env, the running episode's sum of every reward term -- the `info` dictionary of the reference's env.step
        (robots/robot_base.py:88-96) -- and add it to global sums where the episode ends.  Arming zeroes all sums."""
        self._check(self._L.lhw_env_enable_term_stats(self._h, int(bool(enable))))

    def pop_term_sums(self):
        """(term sums [n_terms] float64 over the episodes finished since the last call, terminated, truncated): the raw counters
        (what data-parallel ranks add up); running episodes keep their partial sums."""
        s = np.zeros(self.n_terms)
        ep, te, tr = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        self._check(self._L.lhw_env_pop_term_stats(self._h, s.ctypes.data, ctypes.byref(ep), ctypes.byref(te), ctypes.byref(tr)))
        return s, te.value, tr.value

    def pop_term_stats(self) -> dict:
        """dict(episodes, terminated, truncated, terms={name: mean episode sum}) of the episodes finished since the last call."""
        return term_stats_dict(*self.pop_term_sums(), REWARD_TERMS[self.task])

    def phase_cycles(self, enable=True):
        """Per-phase shader-clock cycles of env 0 since the last call (diagnostic, wave-per-env stepper only)."""
        out = np.zeros(16, dtype=np.int64)
        self._check(self._L.lhw_env_phase_cycles(self._h, int(enable), out.ctypes.data))
        return out

    def pop_fault_stats(self):
        """(contact-overflow steps, diverged-env steps) since the last call."""
        a, b = ctypes.c_int64(), ctypes.c_int64()
        self._check(self._L.lhw_env_pop_fault_stats(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def get_actuator_state(self):
        """(positions, velocities, torques) [N, nu] of the actuated joints as of the last forward pass
        (reference robot_interface.py:163-185)."""
        nu = self.act_dim
        out = [np.zeros((self.n_envs, nu)) for _ in range(3)]
        self._check(self._L.lhw_env_get_actuator_state(self._h, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data))
        return tuple(out)

    def enable_task_inputs(self, enable: bool = True):
        """Arm / disarm the batched sim facade (include/lhw.h: LhwTaskInput): from the next control step on the kernel exports,
        per env, what the reference's tasks read through RobotInterface and what RobotBase.step passes to calc_reward."""
        self._check(self._L.lhw_env_enable_task_inputs(self._h, int(bool(enable))))

    def get_task_inputs(self) -> dict:
        """Named float64 arrays of the last control step's task inputs (host copy, synchronous)."""
        rec = np.zeros((self.n_envs, _lib.TASK_INPUT_DIM))
        self._check(self._L.lhw_env_get_task_inputs(self._h, rec.ctypes.data))
        return _lib.split_task_inputs(rec, self.nq, self.nv, self.act_dim)

    def enable_step_task_inputs(self, enable: bool = True):
        """Arm / disarm the stepping task's second record (include/lhw.h: LhwStepTaskInput; jvrc_step only): foot force sites,
        footstep targets, the target state machine and the root quaternion of every control step from the next one on."""
        self._check(self._L.lhw_env_enable_step_task_inputs(self._h, int(bool(enable))))

    def get_step_task_inputs(self) -> dict:
        """Named float64 arrays of the last control step's stepping record (host copy, synchronous)."""
        rec = np.zeros((self.n_envs, _lib.STEP_TASK_INPUT_DIM))
        self._check(self._L.lhw_env_get_step_task_inputs(self._h, rec.ctypes.data))
        return _lib.split_step_task_inputs(rec)

    def wave_cycles(self):
        """Per-env shader-clock cycles of the last control-step launch (diagnostic; the first call only arms the recording)."""
        out = np.zeros(self.n_envs, dtype=np.int64)
        self._check(self._L.lhw_env_debug_wave_cycles(self._h, out.ctypes.data))
        return out

    def pop_rerun_count(self):
        """Control steps since the last call that needed the one-env-per-wave re-run (more than 8 contacts)."""
        a = ctypes.c_int64()
        self._check(self._L.lhw_env_pop_rerun_count(self._h, ctypes.byref(a)))
        return a.value

    def debug_step_record(self):
        """Stepping task test hook: (sequence [N,20,6] = x y z theta cos sin, floor_z [N], istate [N,5] = t1 t2 reached frames nseq)."""
        seq = np.zeros((self.n_envs, 20, 6))
        fz = np.zeros(self.n_envs)
        ist = np.zeros((self.n_envs, 5), np.int32)
        self._check(self._L.lhw_env_debug_step_record(self._h, seq.ctypes.data, fz.ctypes.data, ist.ctypes.data))
        return seq, fz, ist

    def set_iteration(self, it: int):
        self._check(self._L.lhw_env_set_iteration(self._h, int(it)))
