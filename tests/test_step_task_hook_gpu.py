"""The stepping task as a plug-in on the GPU (task_hook.VectorSteppingTask; include/lhw.h: LhwStepTaskInput): training jvrc_step
through the hook must reproduce the fused task (rewards 1e-6, the kernel's own flags, weights 3e-6) on the resident rollout -- one
launch per rollout, both records of every control step exported, unqueued and through the job queue -- on the launch-per-step
pipeline, and with the task deciding terminations itself.  Reference: robots/robot_base.py:88-96, tasks/stepping_task.py:66-123,
209-262.  CPU twin: tests/test_step_task_hook.py."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _args(N, T):
    return SimpleNamespace(gamma=0.99, lam=0.95, lr=3e-4, eps=1e-5, entropy_coeff=0.0, clip=0.2, minibatch_size=N * T // 2, epochs=2,
                           max_traj_len=T, num_procs=N, num_envs=N, max_grad_norm=0.5, mirror_coeff=0.4, eval_freq=10**9,
                           recurrent=False, imitate=None, learn_std=False, std_dev=0.3, no_mirror=False, continued=None,
                           logdir="/tmp/lhw_test_step_hook", device_index=0)


def _train(task, iters=2, N=24, T=10, env="jvrc_step"):
    from learninghumanoidwalking_amd.envs import ENVIRONMENTS
    from learninghumanoidwalking_amd.ppo import PPO
    algo = PPO(ENVIRONMENTS[env], _args(N, T), seed=5, task=task)
    rews, dones, stats = [], [], []
    for itr in range(iters):
        algo.iterate(itr)
        rews.append(algo.rollout.rew.clone())
        dones.append(algo.rollout.done.clone())
        stats.append(algo._ep_stats)
    return algo, rews, dones, stats


def _same_training(ref, other):
    (fa, rf, df, sf), (oa, ro, do, so) = ref, other
    for a, b in zip(rf, ro):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=0, atol=1e-6)
    for a, b in zip(df, do):
        assert torch.equal(a, b)
    for a, b in zip(sf, so):
        np.testing.assert_allclose(a, b, rtol=1e-6, atol=1e-5)
    np.testing.assert_allclose(oa.kernels.theta.cpu().numpy(), fa.kernels.theta.cpu().numpy(), rtol=0, atol=3e-6)


def test_training_through_the_stepping_hook_reproduces_the_fused_task(monkeypatch):
    from learninghumanoidwalking_amd.task_hook import VectorSteppingTask
    fused = _train(None)
    assert fused[0].rollout.last_mode == "resident"
    vect = _train(lambda spec, dev: VectorSteppingTask(spec, dev))                                   # reward-only, resident
    own = _train(lambda spec, dev: VectorSteppingTask(spec, dev, min_root_height=0.6000001))        # deciding terminations itself
    monkeypatch.setenv("LHW_ROLLOUT_MODE", "steps")
    stp = _train(lambda spec, dev: VectorSteppingTask(spec, dev))                                    # reward-only, launch per step
    monkeypatch.delenv("LHW_ROLLOUT_MODE")
    monkeypatch.setenv("LHW_ROLLOUT_SLOTS", "4")                                                     # 24 groups > 4 slots: the job queue
    monkeypatch.setenv("LHW_ROLLOUT_CHUNK", "3")
    que = _train(lambda spec, dev: VectorSteppingTask(spec, dev))
    assert que[0].env.last_rollout_queued()
    monkeypatch.delenv("LHW_ROLLOUT_SLOTS")
    monkeypatch.delenv("LHW_ROLLOUT_CHUNK")
    assert vect[0].rollout.last_mode == que[0].rollout.last_mode == "resident" and vect[0].rollout.reward_only
    assert own[0].rollout.last_mode == stp[0].rollout.last_mode == "hooked" and not own[0].rollout.reward_only
    for other in (vect, own, stp, que):
        _same_training(fused, other)
    assert any((d != 0).any() for d in fused[2]), "no episode ended"


def test_a_changed_step_reward_weight_changes_what_the_policy_is_trained_on():
    from learninghumanoidwalking_amd.task_hook import VectorSteppingTask
    base, rb, _, _ = _train(lambda spec, dev: VectorSteppingTask(spec, dev), iters=1)
    heavy, rh, _, _ = _train(lambda spec, dev: VectorSteppingTask(spec, dev, weights=dict(step_reward=0.9)), iters=1)
    assert heavy.rollout.last_mode == "resident"
    diff = (rh[0] - rb[0]).cpu().numpy()
    assert (diff > 0).all() and diff.max() <= 0.45 + 1e-6          # 0.45 x a term in (0, 1] more, everywhere
    assert not torch.equal(base.kernels.theta, heavy.kernels.theta)


def test_step_task_inputs_device_view_is_the_host_copy():
    from learninghumanoidwalking_amd.envs.jvrc_step import JvrcStepSpec
    from learninghumanoidwalking_amd.task_hook import device_task_inputs
    spec = JvrcStepSpec()
    env = spec.make_batched(6, seed=3, device=0)
    env.reset()
    ti = device_task_inputs(env)
    assert ti.srec is not None and ti.srec.shape == (6, 32)
    for _ in range(2):
        env.step(torch.randn(6, 12, device="cuda") * 0.2)
    for k, v in env.get_step_task_inputs().items():
        np.testing.assert_array_equal(getattr(ti, k).cpu().numpy(), v, err_msg=k)
    for k, v in env.get_task_inputs().items():
        np.testing.assert_array_equal(getattr(ti, k).cpu().numpy(), v, err_msg=k)
    np.testing.assert_array_equal(ti.goal.float().cpu().numpy(), env.obs[:, 31:39].cpu().numpy())


@pytest.mark.parametrize("queued", [False, True])
def test_resident_step_record_equals_the_per_step_record(monkeypatch, queued):
    """lhw_env_rollout_step_task_inputs against the launch-per-step pipeline replaying the resident rollout's actions: both records
    of every control step bitwise, across truncations / auto-resets; unqueued and through the job queue."""
    from learninghumanoidwalking_amd import _lib
    from learninghumanoidwalking_amd.envs import ENVIRONMENTS
    from learninghumanoidwalking_amd.envs.jvrc_step import JvrcStepSpec
    from learninghumanoidwalking_amd.ppo import PPO
    N, T = 40, 9
    if queued:
        monkeypatch.setenv("LHW_ROLLOUT_SLOTS", "8")
        monkeypatch.setenv("LHW_ROLLOUT_CHUNK", "4")
    algo = PPO(ENVIRONMENTS["jvrc_step"], _args(N, T), seed=2)
    k = algo.kernels
    spec = JvrcStepSpec()
    envs = [spec.make_batched(N, seed=11, device=0, max_traj_len=4) for _ in range(2)]
    obs0 = [e.reset().clone() for e in envs]
    dev = obs0[0].device
    obs = torch.zeros(T + 1, N, spec.obs_dim, device=dev)
    obs[0] = obs0[0]
    act = torch.zeros(T, N, spec.act_dim, device=dev)
    logp, rew = torch.zeros(T, N, device=dev), torch.zeros(T, N, device=dev)
    tob = torch.zeros(T, N, spec.obs_dim, device=dev)
    done = torch.zeros(T, N, dtype=torch.uint8, device=dev)
    tin = torch.full((T, N, _lib.TASK_INPUT_DIM), float("nan"), dtype=torch.float64, device=dev)
    stin = torch.full((T, N, _lib.STEP_TASK_INPUT_DIM), float("nan"), dtype=torch.float64, device=dev)
    k.begin_rollout()
    try:
        pol = k.rollout_policy(seed=1, counter=0, deterministic=False)
        assert envs[0].rollout(pol, T, obs, act, logp, tob, rew, done, task_inputs=tin, step_task_inputs=stin)
    finally:
        k.end_rollout()
    torch.cuda.synchronize()
    assert envs[0].last_rollout_queued() == queued
    e = envs[1]
    e.enable_task_inputs(True)
    e.enable_step_task_inputs(True)
    assert (e.nq, e.nv, e.act_dim) == (19, 18, 12)      # the widths of LhwTaskInput's vectors: the named fields are every used column
    for t in range(T):
        o, r, d, _ = e.step(act[t])
        assert torch.equal(o, obs[t + 1]) and torch.equal(r, rew[t]) and torch.equal(d, done[t])
        srec = np.concatenate([v.reshape(N, -1) for v in e.get_step_task_inputs().values()], axis=1)
        np.testing.assert_array_equal(srec, stin[t, :, :31].cpu().numpy(), err_msg=f"t={t}")
        assert not stin[t, :, 31].any()
        rec, want = e.get_task_inputs(), _lib.split_task_inputs(tin[t].cpu().numpy(), e.nq, e.nv, e.act_dim)
        assert set(rec) == set(_lib.TASK_INPUT_FIELDS)
        for name in rec:
            np.testing.assert_array_equal(rec[name], want[name], err_msg=f"{name} t={t}")
    assert ((done & 2) != 0).any()


def test_walking_task_on_the_stepping_env_decides_its_own_terminations():
    """VectorWalkingTask's done() is not jvrc_step's fused termination: plugged in there, it runs step by step (the rollout truncates
    and resets) even though the task calls itself reward-only."""
    from learninghumanoidwalking_amd.task_hook import VectorWalkingTask
    algo, rews, dones, _ = _train(lambda spec, dev: VectorWalkingTask(spec, dev), iters=1)
    assert algo.task.reward_only and not algo.rollout.reward_only
    assert algo.rollout.last_mode == "hooked"
    assert torch.isfinite(rews[0]).all()
