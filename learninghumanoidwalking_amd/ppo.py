"""PPO learner with on-device rollouts: the host side of the hot path.

Mirrors the reference's learner surface (reference rl/algos/ppo.py:27-641): ``PPO(env_fn, args,
seed)``, ``sample_parallel_with_workers()``, ``update_actor_critic(...)``, ``train(env_fn, n_itr)``
with the same stdout lines and checkpoint names -- but the actor-parallel Ray rollout
(rl/workers/rollout_worker.py) is replaced by one batched environment per GPU, and every
arithmetic step (policy/critic forward, env step, GAE, losses, backward, clip, Adam) runs in
liblhw.so.  Only gradients cross GPUs (``torch.distributed`` all-reduce, RCCL over xGMI).
"""
from __future__ import annotations

import datetime
import os
import sys
import time
from dataclasses import dataclass
from pathlib import Path

import numpy as np
import torch

from . import _lib, dist_utils
from .batched_env import REWARD_TERMS, TASK_JVRC_STEP, term_stats_dict
from .ppo_kernels import PpoKernels, reference_init
from .task_hook import reward_only_on


@dataclass
class BatchData:
    """Same fields as the reference's BatchData (rl/storage/rollout_storage.py:6-22); device tensors."""
    states: torch.Tensor
    actions: torch.Tensor
    rewards: torch.Tensor
    values: torch.Tensor
    returns: torch.Tensor
    dones: torch.Tensor
    traj_idx: torch.Tensor
    ep_lens: torch.Tensor
    ep_rewards: torch.Tensor
    n_envs: int = 0          # > 0: the sample tensors are TIME-major ([T][N] flattened) and traj_idx indexes env_major()

    def env_major(self) -> "BatchData":
        """The same batch with the samples in ENV-major order (sample (env n, step t) at n * T + t): one env's steps are contiguous,
        so `states[traj_idx[i]:traj_idx[i + 1]]` is trajectory i, as with the reference's concatenated worker buffers."""
        if not self.n_envs:
            return self
        N = self.n_envs
        tr = lambda x: x.reshape(-1, N, *x.shape[1:]).transpose(0, 1).reshape(x.shape)
        return BatchData(states=tr(self.states), actions=tr(self.actions), rewards=tr(self.rewards), values=tr(self.values),
                         returns=tr(self.returns), dones=tr(self.dones), traj_idx=self.traj_idx, ep_lens=self.ep_lens,
                         ep_rewards=self.ep_rewards, n_envs=0)


class _AdamView:
    """`actor_optimizer` / `critic_optimizer` of the reference (torch.optim.Adam over the two networks, ppo.py:128-129) as a
    read-only view: one fused Adam kernel updates the flat parameter vector, its moments live in the kernels' adam_m / adam_v."""

    def __init__(self, kernels, names, lr, eps):
        self._k, self._names = kernels, names
        self.defaults = dict(lr=lr, betas=(0.9, 0.999), eps=eps, weight_decay=0)
        self.param_groups = [dict(self.defaults, params=list(names))]

    def state_dict(self):
        k = self._k
        state = {n: dict(step=int(k.adam_step), exp_avg=k._view(k.adam_m, n).detach().cpu().clone(),
                         exp_avg_sq=k._view(k.adam_v, n).detach().cpu().clone()) for n in self._names}
        return dict(state=state, param_groups=[dict(self.defaults, params=list(self._names))])

    def zero_grad(self):      # gradients are zeroed by the apply kernel after every optimiser step
        pass


class RunningMeanStd:
    """Chan parallel mean/variance (reference rl/envs/normalize.py:4-61)."""

    def __init__(self, epsilon=1e-4, shape=()):
        self.mean = np.zeros(shape, dtype=np.float64)
        self.var = np.ones(shape, dtype=np.float64)
        self.count = epsilon

    def update_from_moments(self, batch_mean, batch_var, batch_count):
        delta = batch_mean - self.mean
        tot = self.count + batch_count
        self.mean = self.mean + delta * batch_count / tot
        M2 = self.var * self.count + batch_var * batch_count + np.square(delta) * self.count * batch_count / tot
        self.var = M2 / tot
        self.count = tot

    def update(self, x):
        x = np.asarray(x)
        self.update_from_moments(x.mean(axis=0), x.var(axis=0), x.shape[0])

    @property
    def std(self):
        return np.sqrt(self.var + 1e-8)


def _dist():
    import torch.distributed as dist
    return dist if dist.is_available() and dist.is_initialized() else None


class _RolloutStorage:
    """Time-major rollout storage of one GPU (N envs x T steps per iteration) and the episode carry-over every policy kind shares.

    Semantics of RolloutWorker.sample (reference rl/workers/rollout_worker.py:97-199) for every env:
    exactly T transitions per call, episodes carried over between calls, truncation at max_traj_len,
    bootstrap (not done) * V(s') at episode ends and V(s_T) where the buffer fills mid-episode.
    """

    def __init__(self, env, kernels, T: int, seed: int = 0):
        self.env, self.k, self.T, self.seed = env, kernels, int(T), int(seed)
        N, D, A, dev = env.n_envs, env.obs_dim, env.act_dim, env.device
        self.N = N
        self.obs = torch.zeros(T + 1, N, D, dtype=torch.float32, device=dev)
        self.act = torch.zeros(T, N, A, dtype=torch.float32, device=dev)
        self.logp = torch.zeros(T, N, dtype=torch.float32, device=dev)
        self.val = torch.zeros(T, N, dtype=torch.float32, device=dev)
        self.rew = torch.zeros(T, N, dtype=torch.float32, device=dev)
        self.done = torch.zeros(T, N, dtype=torch.uint8, device=dev)
        self.vterm = torch.zeros(T, N, dtype=torch.float32, device=dev)
        self.vfinal = torch.zeros(N, dtype=torch.float32, device=dev)
        self.counter = 0
        self.started = False
        self.env_base = getattr(env, "env_id_base", 0)      # (a host-only stand-in env may have none)

    def _start(self):
        """The envs are reset once, before the first rollout; afterwards a rollout starts from the last observation of the previous one."""
        if not self.started:
            self.obs[0].copy_(self.env.reset())
            self.started = True
        else:
            self.obs[0].copy_(self.obs[self.T])

    def pop_episode_stats(self):
        """(sum of finished-episode returns, sum of their lengths, their number) since the last call: the env's own counters."""
        return self.env.pop_episode_stats()

    @staticmethod
    def _rollout_mode():
        """LHW_ROLLOUT_MODE: auto | resident (declining raises) | steps (and anything else)"""
        return os.environ.get("LHW_ROLLOUT_MODE", "auto")

    @staticmethod
    def _declined(mode, why) -> bool:
        """The resident rollout is not to be had, because `why`: False -- the launch-per-step pipeline runs -- unless the mode insists on it."""
        if mode == "resident":
            raise _lib.LhwError(-4, f"LHW_ROLLOUT_MODE=resident, but {why}")
        return False


class Rollout(_RolloutStorage):
    """Feed-forward policies: the resident rollout where the library has it, else one policy and one env launch per control step.

    `task`: a task_hook.VectorTask evaluated OUTSIDE the kernels.  A reward-only task keeps the env's fused termination, truncation
    and resets and only replaces the reward; any other task decides terminations itself after every control step, and the rollout,
    not the env, truncates at max_traj_len and resets."""

    def __init__(self, env, kernels: PpoKernels, T: int, seed: int = 0, task=None, max_traj_len: int | None = None):
        super().__init__(env, kernels, T, seed)
        self.task, self.max_traj_len = task, int(max_traj_len if max_traj_len is not None else T)
        self.record_task_inputs = False      # True: a resident rollout also keeps the task-input record of every control step (tin_all)
        # True, on the stepping env without a plugged-in task: the rollout runs launch per step (bitwise the resident one), keeps both
        # task-input records of every control step and the stepping terrain that was in force during it (terrain_seq / _nseq / _floor_z)
        self.record_terrain = False
        self.terrain_seq = self.terrain_nseq = self.terrain_floor_z = None
        # (reward_only is honoured only where the task's done() is this env's fused termination: task_hook.reward_only_on)
        # ... against the bounds the env is configured with (a stand-in env without task_shaping: the reference's)
        shaping = getattr(env, "task_shaping", None) if task is not None else None
        self.reward_only = reward_only_on(task, env.task, shaping()[1] if shaping is not None else None)
        if task is not None and env.history_len > 1 and not self.reward_only:
            # (a task that decides terminations resets through env.reset(mask, obs_out=...), which writes base rows and knows nothing of the
            #  history; a reward-only task leaves flags, resets and with them the history to the kernels, resident or launch per step)
            raise NotImplementedError("a plugged-in task that decides terminations itself is not supported with obs_history_len > 1")
        N, D, dev = self.N, env.obs_dim, env.device
        self.tob_all = torch.zeros(T, N, D, dtype=torch.float32, device=dev)      # [T][N][D] terminal observations
        # Number of independent env groups pipelined on separate streams (wave-per-env steppers; LHW_ROLLOUT_GROUPS overrides).
        # Two groups: one group's policy launch and the tail of its control-step kernel -- a launch ends with its slowest wave,
        # the chip draining meanwhile -- hide behind the other group's kernel.  Measured on the round-4 kernels
        # (profiles/r04_rollout_groups.txt): jvrc_walk @ 4096 +11-12 % env-steps/s over one group
        # (rollout 0.608 -> 0.538 s), h1 @ 4096 +11 %, jvrc_walk @ 2048 / 1024 +4 / +3 %; three or four groups lose badly
        # (jvrc_walk @ 4096: 1.07 s).  (An earlier round had measured one group ahead at 4096 envs, 2.07 vs 1.99 M, on a
        # slower control step and an unfused policy step.)  Small batches keep one group: their launches are latency-bound.
        # Only the plain launch-per-step path uses the groups; with a task plugged in the batch is one group on the current stream.
        want = int(os.environ.get("LHW_ROLLOUT_GROUPS", "2" if N >= 1024 else "1"))
        self.groups = max(1, min(want, N)) if env.task != 0 else 1
        self.streams = None      # (created by the first grouped rollout)
        # plug-in state: episodes carried between rollouts, finished-episode statistics, and the rows the env step writes its own
        # reward (and, hooked, flags) to where the task's replace them
        self._traj_len = torch.zeros(N, dtype=torch.int32, device=dev)
        self._ep_ret = torch.zeros(N, dtype=torch.float64, device=dev)
        self._stats = torch.zeros(3, dtype=torch.float64, device=dev)      # sum of returns, sum of lengths, episodes
        self._scratch_rew = torch.zeros(N, dtype=torch.float32, device=dev)
        self._scratch_done = torch.zeros(N, dtype=torch.uint8, device=dev)
        # the resident rollout's record of every control step for a reward-only task, [T][N][176] float64 -- 2.3 GB at 4096 envs x
        # T = 400 -- and on the stepping env its stepping record, [T][N][32]: allocated by the first resident rollout that needs them
        self._tin_all = self._stin_all = None
        self._rare_path_warm = False

    @property
    def tin_all(self):
        """[T][N][TASK_INPUT_DIM] float64 record of the last resident rollout (None unless one exported it: record_task_inputs or a
        reward-only task)"""
        return self._tin_all if getattr(self, "last_mode", None) in ("resident", "recorded") else None

    @property
    def stin_all(self):
        """[T][N][STEP_TASK_INPUT_DIM] float64 stepping record of the last rollout that exported it (stepping env only), else None"""
        return self._stin_all if getattr(self, "last_mode", None) in ("resident", "recorded") else None

    def collect(self, deterministic=False):
        self._start()
        # Only the actor sits on the step-to-step dependency chain.  The critic's weights do not change during a rollout
        # and it is feed-forward, so V(s_t), V(terminal obs) and V(s_T) are evaluated afterwards in large batches instead
        # of two extra 3-GEMM passes per control step (same values, ~2000 fewer kernel launches per iteration).
        self.k.begin_rollout()      # theta is frozen for the whole rollout (policy steps and the batched critic passes behind them)
        try:
            if not self._rare_path_warm:
                self._warm_rare_path()
            self._collect(deterministic)
            self._critic_values()
        finally:
            self.k.end_rollout()

    def _collect(self, deterministic):
        """Fills obs / act / logp / tob_all / rew / done and sets last_mode: which path collected the rollout (tests, bench line)."""
        T = self.T
        hooked = self.task is not None and not self.reward_only
        if self.record_terrain and self.task is None and self.env.task == TASK_JVRC_STEP:
            self.last_mode = "recorded"
            self._collect_recorded(deterministic)
        elif not hooked and self._collect_resident(deterministic, task_inputs=self.reward_only or self.record_task_inputs):
            self.last_mode = "resident"
            if self.reward_only:
                self._evaluate_recorded_rewards()
        elif self.task is None:
            self.last_mode = "steps"
            self._collect_steps(deterministic, self.rew, self.done)
        else:
            from .task_hook import device_task_inputs
            self.last_mode = "hooked"
            ti = device_task_inputs(self.env)      # (arms the export before the first control step)
            if self.reward_only:      # the kernel's own flags and resets, the task's reward per control step, no host round trip
                self._collect_steps(deterministic, [self._scratch_rew] * T, self.done,
                                    lambda t: self.rew[t].copy_(self._evaluate_reward_batch(ti.rec, ti.srec)))
            else:
                self._collect_steps(deterministic, [self._scratch_rew] * T, [self._scratch_done] * T, lambda t: self._task_step(t, ti))
        if self.reward_only:
            self._episode_stats_from_buffers()

    def _collect_resident(self, deterministic, task_inputs=False) -> bool:
        """All T control steps in one launch, the actor evaluated inside the stepper's wavefronts (BatchedEnv.rollout): bitwise the
        values of the launch-per-step loop (float32 inference; with fp16 inference float32-rounding-close), without its per-control-step
        barrier across the envs.  `task_inputs`: the launch also exports the task-input record(s) of every control step
        (lhw_env_rollout_task_inputs), for a reward-only task evaluated behind it -- RobotBase.step's `task.calc_reward`
        (robots/robot_base.py:88-96) moved behind the rollout, which it may be because a reward does not feed back into the simulation.
        LHW_ROLLOUT_MODE = auto (default: resident wherever the library has the kernel) | resident (declining raises) | steps.
        Returns False where the launch-per-step pipeline is to run instead."""
        # Measured, same box, interleaved (profiles/r05_rollout_modes.txt, final kernels): resident over launch-per-step with two groups --
        # jvrc_walk @ 4096 +25 % env-steps/s (rollout 0.524 -> 0.397 s), jvrc_step @ 4096 +26 %, h1_walk @ 8192 +9 %, h1 @ 8192 +2 %
        # (twice as many wavefronts as the chip holds and a narrow spread of wave times: there two whole-chip launches in flight
        # already backfill each other's tails).
        # An env with an observation history goes the same way (lhw_env_rollout_history): jvrc_walk @ 4096 with obs_history_len 3, sampling
        # 0.47 -> 0.31 s per iteration, resident's mean below every launch-per-step iteration (profiles/r09_history_rollout_ab.txt).
        # Rows past 256 padded columns (up to 1024: the in-wave step takes them in chunks) too: obs_history_len 12, 448 columns, 0.49 - 0.50 ->
        # 0.32 s, by the same rule (profiles/r16_history_long_ab.txt) -- so nothing here asks for the row's width.
        mode = self._rollout_mode()
        if mode not in ("auto", "resident"):
            return False
        env, T = self.env, self.T
        pol = self.k.rollout_policy(seed=self.seed, counter=self.counter, deterministic=deterministic)
        if pol is None:
            return self._declined(mode, "the kernels have no in-wave policy step for this actor")
        if env.env_id_base != self.env_base:
            # (the in-wave policy step keys its noise by the env's own global ids; the per-step calls pass self.env_base + row)
            return self._declined(mode, "the env's env_id_base is not the rollout's")
        if task_inputs and self._tin_all is None:
            self._tin_all = _lib.empty(T, self.N, _lib.TASK_INPUT_DIM, dtype=torch.float64, device=self.obs.device)
            if env.task == TASK_JVRC_STEP:
                self._stin_all = _lib.empty(T, self.N, _lib.STEP_TASK_INPUT_DIM, dtype=torch.float64, device=self.obs.device)
        if not env.rollout(pol, T, self.obs, self.act, self.logp, self.tob_all, self.rew, self.done,
                           task_inputs=self._tin_all if task_inputs else None, step_task_inputs=self._stin_all if task_inputs else None):
            return self._declined(mode, "the library has no resident rollout kernel for this env / policy")
        self.counter += T
        return True

    def _collect_recorded(self, deterministic):
        """The stepping env, launch per step, with a record of everything a frame of it needs: after every control step the two device
        task-input records go to tin_all[t] / stin_all[t], and the host reads the env's footstep sequence (BatchedEnv.debug_step_record:
        a small copy per step at eval batch sizes).  The terrain of step t is the sequence that was IN FORCE DURING control step t: the one
        read after the initial reset for t = 0 and after step t - 1 otherwise -- the one read after step t belongs, at a step that ends
        an episode, to the next episode already."""
        from .task_hook import device_task_inputs
        env, T, N = self.env, self.T, self.N
        ti = device_task_inputs(env)      # (arms both exports before the first control step)
        if self._tin_all is None:
            self._tin_all = _lib.empty(T, N, _lib.TASK_INPUT_DIM, dtype=torch.float64, device=self.obs.device)
            self._stin_all = _lib.empty(T, N, _lib.STEP_TASK_INPUT_DIM, dtype=torch.float64, device=self.obs.device)
        self.terrain_seq, self.terrain_nseq, self.terrain_floor_z = np.zeros((T, N, 20, 4)), np.zeros((T, N), dtype=np.int32), np.zeros((T, N))
        torch.cuda.current_stream(self.obs.device).synchronize()
        in_force = [env.debug_step_record()]

        def after_step(t):
            self._tin_all[t].copy_(ti.rec)
            self._stin_all[t].copy_(ti.srec)
            seq, floor_z, istate = in_force[0]
            self.terrain_seq[t], self.terrain_nseq[t], self.terrain_floor_z[t] = seq[:, :, :4], istate[:, 4], floor_z
            torch.cuda.current_stream(self.obs.device).synchronize()
            in_force[0] = env.debug_step_record()

        groups, self.groups = self.groups, 1      # (one group on the current stream: the hook reads the whole batch)
        try:
            self._collect_steps(deterministic, self.rew, self.done, after_step)
        finally:
            self.groups = groups

    def _collect_steps(self, deterministic, rew, done, after_step=None):
        """Launch per control step: the actor, then the env step writing its reward and flags to rew[t] / done[t], then
        `after_step(t)`.  Without a task the batch advances as `groups` env groups, each on its own HIP stream."""
        env, k, T = self.env, self.k, self.T
        G = self.groups if self.task is None else 1
        bounds = [(g * self.N // G, (g + 1) * self.N // G) for g in range(G)]
        streams = [None]      # (one group: the current stream)
        if G > 1:
            # Environments are independent, so the batch is advanced as G groups on their own HIP streams: a group's policy
            # forward waits only for that group's control-step kernel.  Without the batch-wide barrier per control step the
            # tail of one group's kernel (waves that drew more contacts / Newton iterations / a reset) overlaps the other
            # group's work: 3.8 -> 2.9 ms per control step of 4096 envs with two groups.  Every value is unchanged (the RNG is
            # keyed by global env id and step counter, not by launch order).
            main = torch.cuda.current_stream(self.obs.device)
            if self.streams is None:
                self.streams = [torch.cuda.Stream(device=self.obs.device) for _ in range(G)]
            streams = self.streams
            for s in streams:
                s.wait_stream(main)
        for t in range(T):
            for s, (a, b) in zip(streams, bounds):
                with torch.cuda.stream(s):
                    k.forward(self.obs[t, a:b], seed=self.seed, env_id_base=self.env_base + a, counter=self.counter,
                              deterministic=deterministic, want_value=False, want_mu=False, ws_row=a, act=self.act[t, a:b],
                              logp=self.logp[t, a:b])
                    if G > 1:
                        env.step_range(a, b - a, self.act[t], self.obs[t + 1], self.tob_all[t], rew[t], done[t])
                    else:
                        env.step(self.act[t], obs_out=self.obs[t + 1], term_obs_out=self.tob_all[t], rew_out=rew[t], done_out=done[t])
            if after_step is not None:
                after_step(t)
            self.counter += 1
        if G > 1:
            for s in streams:
                main.wait_stream(s)

    def _critic_values(self):
        T, N = self.T, self.N
        self._batched_values(self.obs[:T].reshape(T * N, -1), self.val.reshape(-1))
        # V(terminal observation) is only read where a trajectory was TRUNCATED (max_traj_len) without terminating: the bootstrap
        # of rl/workers/rollout_worker.py:163-190 (lhw_gae: `(f & 1) ? 0 : vterm`).  That is about one row per env and rollout --
        # 0.25 % of the T x N terminal observations at T = max_traj_len = 400 -- so only those rows go through the critic
        # (50 fewer 32768-row passes per iteration at 4096 envs); everywhere else vterm is 0 and unread.
        need = ((self.done & 2) != 0) & ((self.done & 1) == 0)
        idx = torch.nonzero(need.reshape(-1)).reshape(-1)
        self.vterm.zero_()
        if idx.numel():
            vals = _lib.empty(idx.numel(), dtype=torch.float32, device=self.obs.device)
            self._batched_values(self.tob_all.reshape(T * N, -1).index_select(0, idx), vals)
            self.vterm.reshape(-1).index_copy_(0, idx, vals)
        self.k.forward(self.obs[T], want_actor=False, value=self.vfinal)

    def _batched_values(self, obs_flat, out_flat):
        chunk = int(self.k.max_rows)
        for a in range(0, obs_flat.shape[0], chunk):
            b = min(a + chunk, obs_flat.shape[0])
            self.k.forward(obs_flat[a:b], want_actor=False, value=out_flat[a:b])

    def _warm_rare_path(self):
        """Runs the truncated-trajectory branch of _critic_values once on eight dummy rows.  An untrained policy falls long before
        max_traj_len, so that branch is first taken some ten iterations into a run -- and the first call of its torch ops
        (index_select, index_copy_) loads their code objects: 0.1-0.2 s in the middle of that iteration (bench.py's iter_s showed
        it at iteration 10 of every run).  A process start-up cost, paid here before the first rollout instead."""
        self._rare_path_warm = True
        T = self.T
        need = torch.zeros(T * self.N, dtype=torch.bool, device=self.obs.device)
        need[:8] = True
        idx = torch.nonzero(need).reshape(-1)
        vals = _lib.empty(idx.numel(), dtype=torch.float32, device=self.obs.device)
        self._batched_values(self.tob_all.reshape(T * self.N, -1).index_select(0, idx), vals)
        self.vterm.reshape(-1).index_copy_(0, idx, vals)
        self.vterm.zero_()

    # ---- task plug-ins (task_hook.py)
    def _task_step(self, t, ti):
        """After control step t with a task that decides terminations itself: the env's exported task inputs `ti` go to
        `self.task.evaluate`, whose reward and termination are stored; truncation at max_traj_len, the episode statistics and the
        resets (`lhw_env_reset(mask)`: the reset code and random draws of the in-kernel auto-reset) are done here -- RobotBase.step +
        the episode handling of RolloutWorker.sample (robots/robot_base.py:88-96, rl/workers/rollout_worker.py:150-181) with an
        exchangeable task."""
        rew, term = self.task.evaluate(ti)
        # a diverged env (the kernel has sanitised its state, the record is exported before that): the episode ends -- whatever
        # the plugged task's reward looks at
        bad = ~torch.isfinite(rew) | ~torch.isfinite(ti.qpos).all(1) | ~torch.isfinite(ti.qvel).all(1) | ~torch.isfinite(ti.qacc).all(1)
        rew = torch.where(bad, torch.zeros_like(rew), rew)
        term = term.bool() | bad
        self.rew[t].copy_(rew)
        self._traj_len += 1
        self._ep_ret += rew.double()
        trunc = self._traj_len >= self.max_traj_len
        self.done[t].copy_(term.to(torch.uint8) | (trunc.to(torch.uint8) << 1))
        ended = term | trunc
        # (no host round trip per control step: the statistics are masked sums and the reset launch takes the mask as it is --
        # an all-zero mask is a launch whose waves return at once)
        self._stats += torch.stack([(self._ep_ret * ended).sum(), (self._traj_len * ended).sum().double(), ended.sum().double()])
        self.task.reset(ended)
        self.env.reset(ended.to(torch.uint8), obs_out=self.obs[t + 1])      # rows of the other envs are left untouched
        self._traj_len.masked_fill_(ended, 0)
        self._ep_ret.masked_fill_(ended, 0)

    def _evaluate_reward_batch(self, rec, srec=None):
        """The plugged task's reward for [M, TASK_INPUT_DIM] records (and, stepping env, the [M, STEP_TASK_INPUT_DIM] ones of the same
        rows; non-finite -> 0: the kernel ended that episode itself)."""
        from .task_hook import TaskInputs
        env = self.env
        rew, _ = self.task.evaluate(TaskInputs(rec, env.nq, env.nv, env.act_dim, srec))
        return torch.where(torch.isfinite(rew), rew, torch.zeros_like(rew)).float()

    def _evaluate_recorded_rewards(self):
        """A reward-only task over the records the resident rollout exported: ONE evaluation per half a million rows."""
        T, N = self.T, self.N
        rec = self._tin_all.reshape(T * N, -1)
        srec = self._stin_all.reshape(T * N, -1) if self._stin_all is not None else None
        rew = self.rew.reshape(-1)
        chunk = max(N, (1 << 19) // N * N)      # whole time slices, about half a million rows per evaluation
        for a in range(0, rec.shape[0], chunk):
            rew[a:a + chunk] = self._evaluate_reward_batch(rec[a:a + chunk], srec[a:a + chunk] if srec is not None else None)

    def _episode_stats_from_buffers(self):
        """Finished-episode returns / lengths of this rollout from self.rew (the plugged task's rewards) and self.done (the kernel's
        flags), vectorised over [T, N]; episodes carried in from / out to the neighbouring rollouts through _ep_ret / _traj_len."""
        T, N, dev = self.T, self.N, self.obs.device
        ended = self.done != 0
        cc = torch.cumsum(self.rew.double(), dim=0)
        tt = torch.arange(T, device=dev, dtype=torch.int64).unsqueeze(1).expand(T, N)
        last = torch.cummax(torch.where(ended, tt, torch.full_like(tt, -1)), dim=0).values          # last end at or before t
        prev = torch.cat([torch.full((1, N), -1, dtype=torch.int64, device=dev), last[:-1]], dim=0)  # last end strictly before t
        has_prev = prev >= 0
        base = torch.where(has_prev, cc.gather(0, prev.clamp(min=0)), torch.zeros_like(cc))
        ret = cc - base + torch.where(has_prev, torch.zeros_like(cc), self._ep_ret.unsqueeze(0).expand(T, N))
        length = torch.where(has_prev, tt - prev, tt + 1 + self._traj_len.unsqueeze(0).to(torch.int64))
        e = ended.double()
        self._stats += torch.stack([(ret * e).sum(), (length.double() * e).sum(), e.sum()])
        fin = last[-1]                                                                                # last end of the column (-1: none)
        none = fin < 0
        tail = cc[-1] - torch.where(none, torch.zeros_like(cc[-1]), cc.gather(0, fin.clamp(min=0).unsqueeze(0)).squeeze(0))
        self._ep_ret = torch.where(none, self._ep_ret + cc[-1], tail)
        self._traj_len = torch.where(none, self._traj_len.to(torch.int64) + T, (T - 1) - fin).to(torch.int32)

    def pop_episode_stats(self):
        """(sum of finished-episode returns, sum of their lengths, their number) since the last call -- the env's own counters, or,
        with a task plugged in, the rollout's (returns in the plugged task's reward)."""
        if self.task is None:
            return self.env.pop_episode_stats()
        s = self._stats.cpu().numpy()
        self._stats.zero_()
        return float(s[0]), float(s[1]), int(s[2])


# Whether LHW_ROLLOUT_MODE=auto sends an LSTM actor through the resident rollout (RecurrentRollout): decided by the A/B measurement of
# DESIGN.md section 1 (profiles/r07_lstm_resident_ab.txt) under the rule of the term-statistics work -- resident by default only if its
# mean sample time lies below every run of the launch-per-step parent.
LSTM_RESIDENT_AUTO = False
# Whether RecurrentRollout evaluates the critic of a rollout in one launch behind it (RnnKernels.values) instead of per control step:
# LHW_RNN_SEQ_CRITIC = 0 | 1 overrides.  Same bits either way; the A/B of DESIGN.md section 4.2d decides the default under the same rule.
RNN_SEQ_CRITIC_DEFAULT = False


class RecurrentRollout(_RolloutStorage):
    """LSTM policies.  As in the reference's worker (rollout_worker.py:130-190: `current_state` / hidden state are only
    initialised when they are None), episodes AND the LSTM hidden / cell state are carried from one batch to the next:
    the envs are reset once, before the first batch; afterwards a batch starts from the last observation of the previous
    one with the hidden state the previous batch left, zeroed only for envs whose episode ended on its last step.  The
    hidden state advances with every policy / critic call; terminal and final values are evaluated without advancing it.
    (The update, like the reference's, restarts every stored trajectory -- here every env column -- from a zero state.)

    Two ways to collect, bitwise the same buffers (tests/test_rollout_lstm_gpu.py): launch per control step, or the resident rollout
    (BatchedEnv.rollout_lstm: one launch, the actor's two cells evaluated inside the stepper's wavefronts) followed by the critic over
    the stored time slices.  LHW_ROLLOUT_MODE = auto (LSTM_RESIDENT_AUTO decides) | resident (declining raises) | steps; `last_mode`
    names the path the last collect() took.

    The critic: with LHW_RNN_SEQ_CRITIC=1 (read once, here; default RNN_SEQ_CRITIC_DEFAULT) both paths collect with the actor alone and
    evaluate val / vterm / vfinal of the whole rollout in one launch behind it (RnnKernels.values), where the kernel covers the critic's
    shape; otherwise per control step (`forward`).  `last_critic_mode` = "sequence" | "steps" names what the last collect() did."""

    def __init__(self, env, kernels, T: int, seed: int = 0):
        super().__init__(env, kernels, T, seed)
        N, D, A, dev = self.N, env.obs_dim, env.act_dim, env.device
        self.mu = torch.zeros(N, A, dtype=torch.float32, device=dev)      # the last step's means (launch-per-step path only: nothing reads them)
        self.tob = torch.zeros(N, D, dtype=torch.float32, device=dev)
        self._rec_reset = torch.ones(N, dtype=torch.uint8, device=dev)      # every env starts from a zero state
        self.record_task_inputs = False      # True: a resident rollout also keeps the task-input record of every control step (tin_all)
        self._tob_all = self._tin_all = None      # [T][N][D] terminal observations / [T][N][176] records: allocated by the first resident rollout
        self.last_mode = None
        self.seq_critic = os.environ.get("LHW_RNN_SEQ_CRITIC", "1" if RNN_SEQ_CRITIC_DEFAULT else "0") != "0"
        self.last_critic_mode = None

    @property
    def tin_all(self):
        """[T][N][TASK_INPUT_DIM] float64 record of the last resident rollout (None unless one exported it: record_task_inputs)"""
        return self._tin_all if self.last_mode == "resident" else None

    def collect(self, deterministic=False):
        self._start()
        self.last_critic_mode = None      # set by whichever path evaluates val / vterm
        reset0 = self._rec_reset
        if self._collect_resident(deterministic):
            self.last_mode = "resident"
        else:
            self.last_mode = "steps"
            self._collect_steps(deterministic)
        if self.last_critic_mode is None:      # the actor alone has run: the critic over the stored slices, in one launch or step by step
            if self.k.values(self.obs, self._tob_all, self.done, reset0, self.val, self.vterm, self.vfinal):
                self.last_critic_mode = "sequence"
                return
            self._critic_steps(reset0)
        self.k.forward(self.obs[self.T], commit=False, want_actor=False, value=self.vfinal)

    def _critic_steps(self, reset):
        """V(s_t) advancing the critic's state, V(terminal observation) without, over the stored slices: the calls of the launch-per-step loop"""
        k = self.k
        for t in range(self.T):
            k.forward(self.obs[t], reset=reset, commit=True, want_actor=False, value=self.val[t])
            k.forward(self._tob_all[t], commit=False, want_actor=False, value=self.vterm[t])
            reset = (self.done[t] != 0).to(torch.uint8)
        self.last_critic_mode = "steps"

    def _collect_steps(self, deterministic):
        env, k, T = self.env, self.k, self.T
        reset = self._rec_reset
        if self.seq_critic:      # actor only; the terminal observations are kept for the critic's pass behind the loop
            if self._tob_all is None:
                self._tob_all = _lib.empty(T, self.N, env.obs_dim, dtype=torch.float32, device=self.obs.device)
            for t in range(T):
                k.forward(self.obs[t], reset=reset, seed=self.seed, env_id_base=self.env_base, counter=self.counter, deterministic=deterministic,
                          commit=True, want_value=False, mu=self.mu, act=self.act[t], logp=self.logp[t])
                env.step(self.act[t], obs_out=self.obs[t + 1], term_obs_out=self._tob_all[t], rew_out=self.rew[t], done_out=self.done[t])
                reset = (self.done[t] != 0).to(torch.uint8)
                self.counter += 1
            self._rec_reset = reset
            return
        for t in range(T):
            k.forward(self.obs[t], reset=reset, seed=self.seed, env_id_base=self.env_base, counter=self.counter,
                      deterministic=deterministic, commit=True, mu=self.mu, act=self.act[t], logp=self.logp[t], value=self.val[t])
            env.step(self.act[t], obs_out=self.obs[t + 1], term_obs_out=self.tob, rew_out=self.rew[t], done_out=self.done[t])
            k.forward(self.tob, commit=False, want_actor=False, value=self.vterm[t])
            reset = (self.done[t] != 0).to(torch.uint8)
            self.counter += 1
        self._rec_reset = reset
        self.last_critic_mode = "steps"

    def _collect_resident(self, deterministic) -> bool:
        """All T control steps in one launch, then the critic over the stored slices in the order of the launch-per-step loop
        (V(s_t) advancing the critic's state, V(terminal observation) without): the same calls on the same values, so not a bit of
        `val` / `vterm` changes, and the critic no longer sits between two control steps.  The means of the last step (`self.mu`) are
        not produced here: nothing reads them.  Returns False where the launch-per-step loop is to run instead."""
        mode = self._rollout_mode()
        if mode not in ("auto", "resident") or (mode == "auto" and not (LSTM_RESIDENT_AUTO or self.record_task_inputs)):
            return False      # (the per-step record exists only on the resident path: asking for it selects that path)
        env, k, T = self.env, self.k, self.T
        if env.task == 0:
            return self._declined(mode, "the cartpole env has no wave-per-env stepper to host a policy step")
        if k.hidden != 256:
            return self._declined(mode, f"the in-wave LSTM step covers hidden width 256 only (this actor: {k.hidden})")
        if env.env_id_base != self.env_base:
            return self._declined(mode, "the env's env_id_base is not the rollout's")
        if env.history_len > 1:
            return self._declined(mode, "the env keeps an observation history above the kernels")
        pol = k.rollout_policy(seed=self.seed, counter=self.counter, deterministic=deterministic)
        if pol is None:
            return self._declined(mode, "the kernels have no in-wave policy step for this actor")
        if self._tob_all is None:
            self._tob_all = _lib.empty(T, self.N, env.obs_dim, dtype=torch.float32, device=self.obs.device)
        if self.record_task_inputs and self._tin_all is None:
            self._tin_all = _lib.empty(T, self.N, _lib.TASK_INPUT_DIM, dtype=torch.float64, device=self.obs.device)
        if not env.rollout_lstm(pol, T, self.obs, self.act, self.logp, self._tob_all, self.rew, self.done, self._rec_reset,
                                task_inputs=self._tin_all if self.record_task_inputs else None):
            return self._declined(mode, "the library has no resident LSTM rollout kernel for this env / policy")
        if not self.seq_critic:
            self._critic_steps(self._rec_reset)
        self._rec_reset = (self.done[T - 1] != 0).to(torch.uint8)
        self.counter += T
        return True


# Whether a PPO learner arms the per-term episode statistics of its env unless told otherwise (PPO(term_stats=...), --term-stats /
# --no-term-stats, LHW_TERM_STATS=0 / 1): decided by the A/B measurement of DESIGN.md section 1 -- armed, jvrc_walk @ 4096 ran 0.6 % below
# the parent's mean and outside the spread of the parent's own runs, so it is opt-in.
TERM_STATS_DEFAULT = False


class PPO:
    def __init__(self, env_fn, args, seed=None, task=None, term_stats=None):
        """`term_stats`: arm the per-term episode statistics of the env's kernels (BatchedEnv.enable_term_stats): every
        sample_parallel_with_workers() then leaves the statistics of the episodes it finished in `self.term_stats` and train() logs
        them to reward_terms.csv.  None: args.term_stats, else LHW_TERM_STATS, else TERM_STATS_DEFAULT.  With a plugged-in `task` the
        reward does not come from the kernels: the statistics stay off and `term_stats` is None.
        `task`: None -- the task fused into the env's kernels (the reference's own) -- or a callable `task(spec, device)`
        returning a task_hook.VectorTask: reward and termination then come from that object, evaluated outside the kernels on the
        exported task inputs after every control step (feed-forward policies, humanoid envs; see task_hook.py)."""
        self.seed = seed
        self.gamma, self.lam, self.lr, self.eps = args.gamma, args.lam, args.lr, args.eps
        self.ent_coeff, self.clip = args.entropy_coeff, args.clip
        self.minibatch_size, self.epochs = args.minibatch_size, args.epochs
        self.max_traj_len = args.max_traj_len
        # --num-procs keeps its meaning "number of parallel environments" (per GPU) unless --num-envs is given
        self.n_proc = int(getattr(args, "num_envs", None) or args.num_procs)
        self.grad_clip, self.mirror_coeff = args.max_grad_norm, args.mirror_coeff
        self.eval_freq = args.eval_freq
        self.recurrent = bool(getattr(args, "recurrent", False))
        self.imitate_coeff = float(getattr(args, "imitate_coeff", 0.3))
        self.batch_size = self.n_proc * self.max_traj_len
        self.total_steps = 0
        self.iteration_count = 0
        self.save_path = Path(args.logdir)
        self.best_metric = -np.inf
        d = _dist()
        self.rank = d.get_rank() if d else 0
        self.world = d.get_world_size() if d else 1
        if self.rank == 0:
            self.save_path.mkdir(parents=True, exist_ok=True)
        dev_index = getattr(args, "device_index", None)
        if dev_index is None:
            dev_index = torch.cuda.current_device() if torch.cuda.is_available() else 0
        self.device = torch.device("cuda", dev_index)

        spec = env_fn()  # env description object (see envs/*): dims, obs norm, mirror tables, batched factory
        self.spec = spec
        obs_dim, act_dim = spec.obs_dim, spec.act_dim
        mirror = None if getattr(args, "no_mirror", False) else spec.mirror_tables()
        hyper = dict(device=self.device, learn_std=args.learn_std, lr=self.lr, eps=self.eps, clip=self.clip, entropy_coeff=self.ent_coeff,
                     mirror_coeff=self.mirror_coeff, max_grad_norm=self.grad_clip,
                     mirror_obs=mirror[0] if mirror else None, mirror_act=mirror[1] if mirror else None)
        # 1. the kernels, with the checkpoint loader and weight initialisation of the policy kind
        if self.recurrent:
            # LSTM actor / critic (ppo.py:84-86); a minibatch is `minibatch_size` whole env columns of the rollout
            from .checkpoint import load_recurrent_checkpoint as load_checkpoint
            from .rnn_kernels import RnnKernels, reference_init_lstm as init_weights
            hidden = int(getattr(args, "lstm_hidden", 256))
            cols = min(self.n_proc, int(self.minibatch_size or self.n_proc))
            self.kernels = RnnKernels(obs_dim, act_dim, hidden=hidden, seq_len=self.max_traj_len, seq_cols=cols, rollout_rows=self.n_proc,
                                      **hyper)
        else:
            from .checkpoint import load_reference_checkpoint as load_checkpoint
            init_weights, hidden = reference_init, 256
            self.kernels = PpoKernels(obs_dim, act_dim, hidden=hidden, max_rows=max(self.n_proc, int(self.minibatch_size or self.batch_size)),
                                      **hyper)
        # 2. the option combinations the LSTM path does not implement
        fp16, infer_fp16 = getattr(args, "fp16", False), getattr(args, "infer_fp16", False)
        if self.recurrent:
            if getattr(args, "imitate", None):
                raise NotImplementedError("--imitate together with --recurrent is not supported")
            if infer_fp16:
                raise NotImplementedError("--infer-fp16 is implemented for the feed-forward policies")
            if fp16:
                raise NotImplementedError("--fp16 is implemented for the feed-forward policies")
            if task is not None:
                raise NotImplementedError("a plugged-in task needs the feed-forward policies")
        if infer_fp16 or fp16:
            self.kernels.set_inference_fp16(True)   # rollout inference on the fp16 MFMA; the update stays float32
        if fp16:
            # BASELINE config 5: fp16 actor / critic -- inference AND every GEMM of the update with fp16 operands (float32
            # accumulation, master weights, loss and Adam)
            self.kernels.set_update_fp16(True)
        # 3. the weights: --continued actor_X.pt loads the actor + sibling critic, re-initialises stds and keeps the embedded obs
        # normalisation (reference rl/algos/ppo.py:69-82); otherwise identical initial weights on every rank: the reference's init
        # path under a fixed torch seed
        continued = getattr(args, "continued", None)
        if continued:
            cpath = Path(Path(continued).parent, "critic" + str(continued).split("actor")[1])
            t, om, osd = load_checkpoint(continued, cpath)[:3]      # (the LSTM loader also returns the hidden width)
            t["stds"] = args.std_dev * torch.ones(act_dim)
            self.kernels.set_tensors(t)
            self.kernels.set_obs_norm(om.numpy(), osd.numpy())
            self._log("Loaded (pre-trained) actor from: " + str(continued))
            self._log("Loaded (pre-trained) critic from: " + str(cpath))
        else:
            self.kernels.set_tensors(init_weights(obs_dim, act_dim, hidden, args.std_dev, generator_seed=self._init_seed(seed)))
        # 4. observation normalisation: the checkpoint's, the env's fixed one, or a running one warmed up by train()
        self.obs_rms = None
        if continued:
            pass
        elif spec.obs_mean is not None:
            if len(spec.obs_mean) != obs_dim or len(spec.obs_std) != obs_dim:
                raise ValueError(f"{type(spec).__name__}: obs_mean / obs_std have {len(spec.obs_mean)} / {len(spec.obs_std)} entries "
                                 f"for an observation of {obs_dim} (base {getattr(spec, 'base_obs_dim', obs_dim)} x history)")
            self.kernels.set_obs_norm(spec.obs_mean, spec.obs_std)
            self._log("Using fixed observation normalization from environment.")
        else:
            self.obs_rms = RunningMeanStd(shape=(obs_dim,))
            self.kernels.set_obs_norm(self.obs_rms.mean, self.obs_rms.std)
            self._log("Using running observation normalization (will update during training).")
        env_seed = (seed if seed is not None else int(time.time())) & 0x7FFFFFFF
        self.env_seed = env_seed
        self.task = task(spec, self.device) if task is not None else None
        # A task that decides terminations itself is consulted after every control step and the env never ends an episode by itself:
        # the rollout truncates and resets (Rollout._task_step).  A reward-only task leaves all that to the kernel.
        # (reward_only counts only where the task declares this env's fused termination as its own: task_hook.reward_only_on,
        #  and its bounds are the ones this env will be configured with: the YAML's `termination:`, else the reference's)
        shaping = getattr(spec, "task_shaping", lambda: None)()
        own_done = self.task is not None and not reward_only_on(self.task, getattr(spec, "task_code", None), shaping[1] if shaping else None)
        self.env = spec.make_batched(self.n_proc, seed=env_seed, device=self.device, max_traj_len=0 if own_done else self.max_traj_len,
                                     env_id_base=dist_utils.shard_env_ids(self.n_proc, self.rank))
        self.env.env_id_base = dist_utils.shard_env_ids(self.n_proc, self.rank)
        if term_stats is None:
            term_stats = getattr(args, "term_stats", None)
        if term_stats is None:
            term_stats = os.environ.get("LHW_TERM_STATS", "1" if TERM_STATS_DEFAULT else "0") != "0"
        self.term_stats_enabled = bool(term_stats) and self.task is None
        self.term_stats = None
        if self.term_stats_enabled:
            self.env.enable_term_stats(True)
        rollout_seed = env_seed ^ 0x5DEECE66D
        if self.recurrent:
            self.rollout = RecurrentRollout(self.env, self.kernels, self.max_traj_len, seed=rollout_seed)
        else:
            self.rollout = Rollout(self.env, self.kernels, self.max_traj_len, seed=rollout_seed, task=self.task, max_traj_len=self.max_traj_len)
        # --imitate: frozen expert + the env's projector (reference rl/algos/ppo.py:111-122)
        self.base_policy, self.imitation_projector = None, None
        if getattr(args, "imitate", None):
            factory = getattr(spec, "imitation_projector", None)
            projector = factory() if callable(factory) else None
            if projector is None:
                raise ValueError(f"--imitate was passed but env {type(spec).__name__} does not implement "
                                 "imitation_projector(); cannot construct expert query.")
            from .imitation import FrozenActor
            self.base_policy = FrozenActor(args.imitate, self.device, max_rows=self.kernels.max_rows)
            self.imitation_projector = projector
        self.policy = self.kernels  # attribute names the reference's tests look for
        self.critic = self.kernels
        # The reference deep-copies the actor into old_policy every iteration only to evaluate the behaviour log-probs; here
        # they are stored by the rollout (and recomputed in float32 for the fp16-inference mode), so old_policy is the policy.
        self.old_policy = self.kernels
        names = self.kernels.TENSORS
        self.actor_optimizer = _AdamView(self.kernels, [n for n in names if n.startswith("a_") or n == "stds"], self.lr, self.eps)
        self.critic_optimizer = _AdamView(self.kernels, [n for n in names if n.startswith("c_")], self.lr, self.eps)
        self.last_losses = {}

    # ------------------------------------------------------------------ sampling
    def sample_parallel_with_workers(self, deterministic=False) -> BatchData:
        self.env.set_iteration(self.iteration_count)
        ro = self.rollout
        ro.collect(deterministic=deterministic)
        ret, adv = self.kernels.gae(ro.rew, ro.val, ro.done, ro.vterm, ro.vfinal, self.gamma, self.lam)
        self._adv, self._ret = adv, ret
        T, N = ro.T, ro.N
        rs, ls, cnt = ro.pop_episode_stats()
        coll_dev = self.device if _dist() and _dist().get_backend() == 'nccl' else None
        self._ep_stats = dist_utils.global_episode_stats(rs, ls, cnt, device=coll_dev)
        if self.term_stats_enabled:      # per-term sums of the episodes this rollout finished, over all ranks like the episode statistics
            sums = dist_utils.global_term_sums(*self.env.pop_term_sums(), device=coll_dev)
            self.term_stats = term_stats_dict(*sums, REWARD_TERMS[self.env.task])
        return BatchData(states=ro.obs[:T].reshape(T * N, -1), actions=ro.act.reshape(T * N, -1),
                         rewards=ro.rew.reshape(T * N, 1), values=ro.val.reshape(T * N, 1), returns=ret.reshape(T * N, 1),
                         dones=ro.done.reshape(T * N, 1), traj_idx=self._traj_idx(ro.done),
                         ep_lens=torch.tensor([ls / cnt] if cnt else []), ep_rewards=torch.tensor([rs / cnt] if cnt else []), n_envs=N)

    @staticmethod
    def _traj_idx(done):
        """Trajectory boundaries like PPOBuffer.traj_idx (rl/storage/rollout_storage.py:24-51: [0, end of 1st trajectory, ...,
        number of samples]) for the ENV-MAJOR order of the batch -- sample (env n, step t) at n * T + t, i.e.
        `states.view(T, N, -1).transpose(0, 1)`: one env's T steps are contiguous there, and a trajectory ends where that env's
        episode ended or the buffer filled.  (The tensors of BatchData themselves are time-major, [T][N] flattened.)"""
        T, N = done.shape
        ends = (done.t() != 0)                      # [N][T]
        ends[:, T - 1] = True
        idx = torch.nonzero(ends.reshape(-1)).reshape(-1) + 1
        return torch.cat([torch.zeros(1, dtype=idx.dtype, device=idx.device), idx])

    # ------------------------------------------------------------------ update
    def _normalize_advantages(self, adv_flat):
        """(adv - mean) / (unbiased std + eps) over the GLOBAL batch (ppo.py:484-485)."""
        pack = dist_utils.global_moments_pack(self.kernels.moments(adv_flat), adv_flat.numel())   # stays on the device
        self.kernels.standardize(adv_flat, pack, self.eps)

    def update_actor_critic(self, obs_batch, action_batch, return_batch, advantage_batch, mask=1, mirror_observation=None,
                            mirror_action=None, old_log_probs=None):
        """One optimiser step on an explicit minibatch (same 7-tuple as the reference, ppo.py:299-406).
        ``mask`` must be 1 (FF path).  The mirror functions are configured at construction; the
        arguments are accepted for signature compatibility."""
        if self.recurrent:
            raise NotImplementedError("explicit padded-trajectory minibatches are not exposed for the LSTM path; use optimize()")
        k = self.kernels
        obs = obs_batch.to(self.device, torch.float32).contiguous()
        B = obs.shape[0]
        act = action_batch.to(self.device, torch.float32).contiguous()
        if old_log_probs is None:  # the reference recomputes them with old_policy == policy before the first step
            sd = k.get_tensors()["stds"].to(self.device)
            mu, _, _, _ = k.forward(obs, deterministic=True, want_value=False)
            old_log_probs = torch.distributions.Normal(mu, sd).log_prob(act).sum(-1)
        xn, xm = k.normalize(obs)
        k.stats.zero_()
        idx = torch.arange(B, dtype=torch.int32, device=self.device)
        k.grad_minibatch(xn, xm, act, old_log_probs.reshape(-1).to(self.device, torch.float32).contiguous(),
                         advantage_batch.reshape(-1).to(self.device, torch.float32).contiguous(),
                         return_batch.reshape(-1).to(self.device, torch.float32).contiguous(), idx,
                         imitation=self._imitation_term(obs))
        self._allreduce_and_apply()
        s = k.stats.cpu().numpy()
        return (float(s[0]), self._entropy_penalty(), float(s[1]), float(s[3]), float(s[2]), float(s[5]), float(s[4]))

    def _imitation_term(self, obs_mb):
        """Imitation loss inputs of one minibatch of RAW observations (ppo.py:360-368): ask the env's projector what the
        expert should see, run the frozen expert, scatter its means into the dense target the loss kernel reads."""
        if self.imitation_projector is None:
            return None
        from .imitation import dense_imitation_target
        query = self.imitation_projector(obs_mb)
        if not bool(query.sample_mask.any()):
            return None
        target = self.base_policy(query.expert_obs)
        dense, mask, count = dense_imitation_target(query, target, obs_mb.shape[0], self.spec.act_dim)
        return (self.imitate_coeff, dense, mask, count) if count > 0 else None

    def _entropy_penalty(self):
        sd = self.kernels.get_tensors()["stds"].numpy().astype(np.float64)
        return float(-np.mean(0.5 + 0.5 * np.log(2 * np.pi) + np.log(sd)))

    def _allreduce_and_apply(self):
        scale = dist_utils.allreduce_grad_(self.kernels.grad)  # RCCL sum over xGMI: the only data-path collective
        self.kernels.apply(grad_scale=scale)

    def _optimize_recurrent(self, itr: int):
        """Recurrent branch of PPO.train (ppo.py:512-533): `epochs` passes over shuffled minibatches of whole trajectories
        -- here `minibatch_size` env columns of the time-major rollout (each column = back-to-back trajectories, the LSTM
        state is reset where one starts), last partial minibatch kept (drop_last=False) -- BPTT on each."""
        k, ro = self.kernels, self.rollout
        T, N = ro.T, ro.N
        adv = self._adv.reshape(-1)
        self._normalize_advantages(adv)
        ret = self._ret.reshape(-1)
        xn, xm = k.normalize(ro.obs[:T].reshape(T * N, -1))
        act, logp = ro.act.reshape(T * N, -1), ro.logp.reshape(-1)
        mb = min(int(self.minibatch_size or N), N, k.seq_cols)
        k.stats.zero_()
        n_updates = 0
        for epoch in range(self.epochs):
            g = torch.Generator(device=self.device)
            g.manual_seed((self.seed if self.seed is not None else 0) + itr * self.epochs + epoch + 1000003 * self.rank)
            perm = torch.randperm(N, generator=g, device=self.device, dtype=torch.int64).to(torch.int32)
            for start in range(0, N, mb):
                k.grad_columns(T, N, xn, xm, act, logp, adv, ret, ro.done, perm[start:start + mb].contiguous())
                self._allreduce_and_apply()
                n_updates += 1
        s = (k.stats / max(1, n_updates)).cpu().numpy()
        self.last_losses = dict(actor=float(s[0]), critic=float(s[1]), mirror=float(s[2]), kl=float(s[3]), clip_fraction=float(s[4]),
                                imitation=0.0, entropy=self._entropy_penalty(), n_updates=n_updates)
        return self.last_losses

    def optimize(self, itr: int):
        """The per-iteration update of PPO.train (ppo.py:484-566): advantage normalisation, then
        `epochs` passes of shuffled minibatches (drop_last).  Returns dict of mean losses."""
        if self.recurrent:
            return self._optimize_recurrent(itr)
        k, ro = self.kernels, self.rollout
        T, N = ro.T, ro.N
        n_samples = T * N
        adv = self._adv.reshape(-1)
        self._normalize_advantages(adv)
        ret = self._ret.reshape(-1)
        raw_obs = ro.obs[:T].reshape(n_samples, -1)
        xn, xm = k.normalize(raw_obs)
        act = ro.act.reshape(n_samples, -1)
        logp = ro.logp.reshape(-1)
        if getattr(k, "inference_fp16", False) and not getattr(k, "update_fp16", False):
            # (with --fp16 the update evaluates the policy with the same fp16-operand GEMMs as the rollout: nothing to do)
            # The rollout's log-probs came out of the fp16-operand forward; the update evaluates the policy in float32, so
            # ratio != 1 on the very first minibatch from precision noise alone (amplified by 1 / std^2).  The reference
            # evaluates old_policy and policy in the same precision (ppo.py:305-309): recompute the old log-probs once per
            # iteration with the float32 actor, before any weight changes.
            logp = self._float32_log_probs(raw_obs, act)
        mb = int(self.minibatch_size or n_samples)
        mb = min(mb, n_samples)
        k.stats.zero_()
        n_updates = 0
        # Single process, no imitation term: an optimiser step is ONE graph launch (lhw_ppo_step) on a stream of its own -- a hipGraph is
        # captured from a stream, and torch's default stream is the legacy one, which cannot be captured.  With data parallelism the
        # gradient all-reduce sits between the two halves: lhw_ppo_grad, all-reduce, lhw_ppo_apply, eagerly.
        fused = (self.imitation_projector is None and not dist_utils._active(dist_utils.dist())
                 and os.environ.get("LHW_PPO_GRAPH", "1") != "0")
        cur = torch.cuda.current_stream(self.device)
        if fused:
            if getattr(self, "_update_stream", None) is None:
                self._update_stream = torch.cuda.Stream(device=self.device)
            self._update_stream.wait_stream(cur)
        with torch.cuda.stream(self._update_stream if fused else cur):
            for epoch in range(self.epochs):
                perm = self._minibatch_perm(itr, epoch, n_samples)
                for start in range(0, n_samples - mb + 1, mb):
                    mb_idx = perm[start:start + mb]
                    if fused:
                        k.step_minibatch(xn, xm, act, logp, adv, ret, mb_idx)
                    else:
                        imit = self._imitation_term(raw_obs.index_select(0, mb_idx.long())) if self.imitation_projector is not None else None
                        k.grad_minibatch(xn, xm, act, logp, adv, ret, mb_idx, imitation=imit)
                        self._allreduce_and_apply()
                    n_updates += 1
        if fused:
            cur.wait_stream(self._update_stream)
        s = (k.stats / max(1, n_updates)).cpu().numpy()
        self.last_losses = dict(actor=float(s[0]), critic=float(s[1]), mirror=float(s[2]), kl=float(s[3]),
                                clip_fraction=float(s[4]), imitation=float(s[5]), entropy=self._entropy_penalty(), n_updates=n_updates)
        return self.last_losses

    def _minibatch_perm(self, itr, epoch, n_samples, rank=None):
        """Shuffle of this rank's samples for one epoch (per-rank shuffles: statistically, not bitwise, the reference's global
        randperm, ppo.py:487-490); a pure function of (seed, iteration, epoch, rank)."""
        g = torch.Generator(device=self.device)
        base = self.seed if self.seed is not None else 0
        g.manual_seed(base + itr * self.epochs + epoch + 1000003 * (self.rank if rank is None else rank))
        return torch.randperm(n_samples, generator=g, device=self.device, dtype=torch.int64).to(torch.int32)

    def _float32_log_probs(self, obs_flat, act_flat):
        k = self.kernels
        sd = k.get_tensors()["stds"].to(self.device)
        out = _lib.empty(obs_flat.shape[0], dtype=torch.float32, device=self.device)
        k.set_inference_fp16(False)
        try:
            chunk = int(k.max_rows)
            for a in range(0, obs_flat.shape[0], chunk):
                b = min(a + chunk, obs_flat.shape[0])
                mu, _, _, _ = k.forward(obs_flat[a:b], deterministic=True, want_value=False)
                out[a:b] = torch.distributions.Normal(mu, sd).log_prob(act_flat[a:b]).sum(-1)
        finally:
            k.set_inference_fp16(True)
        return out

    def iterate(self, itr: int):
        """One PPO iteration: rollout + GAE + update.  Returns (n_samples_local, sample_time, optimize_time)."""
        self.iteration_count = itr
        t0 = time.time()
        batch = self.sample_parallel_with_workers()
        torch.cuda.synchronize(self.device)
        t1 = time.time()
        self.optimize(itr)
        torch.cuda.synchronize(self.device)
        t2 = time.time()
        return batch, t1 - t0, t2 - t1

    # ------------------------------------------------------------------ checkpoints / eval
    def save(self, itr, metric=None):
        """actor_{itr}.pt / critic_{itr}.pt (+ actor.pt / critic.pt when the metric improves), like
        ModelCheckpointer.save_if_best (reference rl/utils/checkpointer.py:54-83).  The files are whole-module
        pickles naming the reference's classes, so `run_experiment.py eval` / `--continued` of the reference load them."""
        if self.rank != 0:
            return
        from .checkpoint import save_recurrent_checkpoint, save_reference_checkpoint
        write = save_recurrent_checkpoint if self.recurrent else save_reference_checkpoint    # (Gaussian_LSTM_Actor / LSTM_V pickles)
        t = self.kernels.get_tensors()
        om, osd = self.kernels.obs_mean.cpu(), self.kernels.obs_std.cpu()
        write(t, om, osd, self.kernels.learn_std, self.save_path / f"actor_{itr}.pt", self.save_path / f"critic_{itr}.pt")
        if metric is not None and metric > self.best_metric:
            self.best_metric = metric
            write(t, om, osd, self.kernels.learn_std, self.save_path / "actor.pt", self.save_path / "critic.pt")

    def evaluate(self, itr, num_batches=5):
        """5 deterministic batches on the same persistent envs (ppo.py:408-426)."""
        rs = ls = cnt = 0
        for _ in range(num_batches):
            self.sample_parallel_with_workers(deterministic=True)
            r, l, c = self._ep_stats
            rs, ls, cnt = rs + r, ls + l, cnt + c
        mean_r = rs / cnt if cnt else 0.0
        mean_l = ls / cnt if cnt else 0.0
        self.save(itr, mean_r)
        return mean_r, mean_l

    # ------------------------------------------------------------------ training loop
    def _init_seed(self, seed):
        """Seed of the weight initialisation: the run's seed, or -- like the reference without --seed -- a fresh random one
        (rank 0's under torch.distributed, so that every rank starts from the same weights)."""
        if seed is not None:
            return int(seed)
        s = [int.from_bytes(os.urandom(4), "little")]
        d = _dist()
        if d:
            d.broadcast_object_list(s, src=0)
        return s[0]

    def _log(self, msg):
        """progress lines of PPO.train (reference rl/algos/ppo.py:459-566) -- rank 0 only under torch.distributed"""
        if self.rank == 0:
            print(msg)

    def _log_term_stats(self, itr):
        """One row per training iteration in <logdir>/reward_terms.csv -- iteration, episodes, terminated, truncated, then the mean
        episode sum of every reward term: the `info` dictionaries of the reference's env.step (robots/robot_base.py:88-96) that its
        trainer never logs.  Rank 0; nothing is written while the statistics are off.  (stdout keeps the reference's lines.)"""
        s = self.term_stats
        if s is None or self.rank != 0:
            return
        path = self.save_path / "reward_terms.csv"
        new = not path.exists()
        with open(path, "a") as f:
            if new:
                f.write(",".join(["iteration", "episodes", "terminated", "truncated"] + list(s["terms"])) + "\n")
            f.write(",".join([str(itr), str(s["episodes"]), str(s["terminated"]), str(s["truncated"])]
                             + [repr(v) for v in s["terms"].values()]) + "\n")

    def train(self, env_fn, n_itr):
        train_start = time.time()
        k = self.kernels
        if self.obs_rms is not None:
            self._log("Warming up observation normalization...")
            for i in range(5):  # ppo.py:442-457
                batch = self.sample_parallel_with_workers()
                mean, var, n = dist_utils.global_batch_moments(batch.states)  # == update on the concatenated batch
                self.obs_rms.update_from_moments(mean.cpu().numpy(), var.cpu().numpy(), n)
                self._log(f"  Warmup batch {i + 1}: {int(n)} samples, obs_rms count: {self.obs_rms.count:.0f}")
            k.set_obs_norm(self.obs_rms.mean, self.obs_rms.std)
            self._log(f"Normalization initialized with {self.obs_rms.count:.0f} samples")
        for itr in range(n_itr):
            self._log(f"********** Iteration {itr} ************")
            batch, sample_time, optimize_time = self.iterate(itr)
            num_samples = batch.states.shape[0] * self.world
            self._log(f"Sampling took {sample_time:.2f}s for {num_samples} steps.")
            self._log(f"Optimizer took: {optimize_time:.2f}s")
            self.total_steps += num_samples
            L = self.last_losses
            rs, ls, cnt = self._ep_stats
            mean_eprew = rs / cnt if cnt else float("nan")
            mean_eplen = ls / cnt if cnt else float("nan")
            noise = float(np.mean(k.get_tensors()["stds"].numpy()))
            if self.rank == 0:
                w = sys.stdout.write
                w("-" * 37 + "\n")
                w(f"| {'Mean Eprew':>15} | {mean_eprew:>15.5g} |\n")
                w(f"| {'Mean Eplen':>15} | {mean_eplen:>15.5g} |\n")
                w(f"| {'Actor loss':>15} | {L['actor']:>15.3g} |\n")
                w(f"| {'Critic loss':>15} | {L['critic']:>15.3g} |\n")
                w(f"| {'Mirror loss':>15} | {L['mirror']:>15.3g} |\n")
                w(f"| {'Imitation loss':>15} | {L.get('imitation', 0.0):>15.3g} |\n")
                w(f"| {'Mean KL Div':>15} | {L['kl']:>15.3g} |\n")
                w(f"| {'Mean Entropy':>15} | {L['entropy']:>15.3g} |\n")
                w(f"| {'Clip Fraction':>15} | {L['clip_fraction']:>15.3g} |\n")
                w(f"| {'Mean noise std':>15} | {noise:>15.3g} |\n")
                w("-" * 37 + "\n")
                sys.stdout.flush()
            self._log_term_stats(itr)
            total_time = time.time() - train_start
            fps = self.total_steps / total_time
            iter_avg = total_time / (itr + 1)
            eta = round((n_itr - itr) * iter_avg)
            self._log(f"Total time elapsed: {total_time:.2f}s. Total steps: {self.total_steps} "
                      f"(fps={fps:.2f}. iter-avg={iter_avg:.2f}s. ETA={datetime.timedelta(seconds=eta)})")
            if itr == 0 or (itr + 1) % self.eval_freq == 0:
                t0 = time.time()
                mean_r, mean_l = self.evaluate(itr)
                self._log("====EVALUATE EPISODE====")
                self._log(f"(Episode length:{mean_l:.3f}. Reward:{mean_r:.3f}. Time taken:{time.time() - t0:.2f}s)")
