"""The stepping task as a plug-in (task_hook.VectorSteppingTask) and the stepping env's second task-input record (include/lhw.h:
enum LhwStepTaskInput, lhw_env_*step_task_inputs): SteppingTask.calc_reward / done (reference tasks/stepping_task.py:66-123, 249-262)
recomputed outside the kernel must be the reference's own terms on its scripted fixture, and the fused kernel's terms on the record
the kernel exports.  Runs on the SIMT emulator; tests/test_step_task_hook_gpu.py is the GPU twin."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "stepping.npz")


def _records(tin_rows, stin_rows, nq=19, nv=18, nu=12):
    from learninghumanoidwalking_amd.task_hook import TaskInputs
    return TaskInputs(torch.from_numpy(np.ascontiguousarray(tin_rows)), nq, nv, nu, torch.from_numpy(np.ascontiguousarray(stin_rows)))


def test_vector_stepping_task_matches_the_reference_stepping_task():
    """tests/golden/stepping.npz: the reference's SteppingTask executed on scripted kinematics (14 cases x 110 control steps, every walk
    mode); its six terms and done() from the record pair built out of those kinematics and the task state after step()."""
    from learninghumanoidwalking_amd import _lib
    from learninghumanoidwalking_amd.envs.jvrc_step import JvrcStepSpec
    from learninghumanoidwalking_amd.task_hook import VectorSteppingTask
    g = np.load(GOLD)
    tins, stins, rews, dones = [], [], [], []
    F, S = _lib.TASK_INPUT_FIELDS, _lib.STEP_TASK_INPUT_FIELDS
    for n in range(int(g["n"])):
        pre = f"r{n}_"
        kin, tst, seq = g[pre + "kin"], g[pre + "tstate"], g[pre + "sequence"]
        T = len(kin)
        tin, stin = np.zeros((T, _lib.TASK_INPUT_DIM)), np.zeros((T, _lib.STEP_TASK_INPUT_DIM))
        # kin columns (tests/golden/gen_golden.py::gen_stepping): root xpos, head xpos, lf_force, rf_force, root quat, lfoot vel,
        # rfoot vel, l grf, r grf, self collision, min contact z, any foot contact
        col = dict(root_xpos=kin[:, 0:3], head_xpos=kin[:, 3:6], lfoot_vel=kin[:, 16:19], rfoot_vel=kin[:, 19:22], grf_l=kin[:, 22],
                   grf_r=kin[:, 23], self_collision=kin[:, 24], contact_z=kin[:, 25], foot_contact=kin[:, 26], phase=tst[:, 0],
                   mode=np.full(T, g[pre + "in"][0]))
        for k, v in col.items():
            o, w = F[k]
            tin[:, o:o + w] = v.reshape(T, w)
        t1, t2 = tst[:, 1].astype(int), tst[:, 2].astype(int)
        scol = dict(lsite_xpos=kin[:, 6:9], rsite_xpos=kin[:, 9:12], root_xquat=kin[:, 12:16], target1=seq[t1], target2=seq[t2],
                    reached=tst[:, 3], frames=tst[:, 4], t1=t1, t2=t2, nseq=np.full(T, len(seq)), goal=g[pre + "goal"])
        for k, v in scol.items():
            o, w = S[k]
            stin[:, o:o + w] = np.asarray(v, np.float64).reshape(T, w)
        tins.append(tin); stins.append(stin); rews.append(g[pre + "rew"]); dones.append(g[pre + "done"])
    spec = JvrcStepSpec()
    assert spec.period == 88 and spec.goal_height == 0.80
    task = VectorSteppingTask(spec, "cpu")
    assert task.mass == 16062.0        # the fixture's get_robot_mass()
    ti = _records(np.concatenate(tins), np.concatenate(stins))
    reward, done = task.evaluate(ti)
    want = np.concatenate(rews)
    got = np.stack([task.last_terms[k].numpy() for k in task.TERMS], axis=1)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    np.testing.assert_allclose(reward.numpy(), want.sum(1), rtol=1e-12)
    np.testing.assert_array_equal(done.numpy(), np.concatenate(dones).astype(bool))
    assert 0 < done.sum() < len(done) and (ti.reached != 0).any()


def _step_record(env):
    """the raw [N][32] record: column 31 is reserved, and BatchedEnv.get_step_task_inputs returns the named fields only"""
    rec = np.zeros((env.n_envs, 32))
    assert env._L.lhw_env_get_step_task_inputs(env._h, rec.ctypes.data) == 0, env._L.lhw_last_error()
    return rec


def _task_record(env):
    from learninghumanoidwalking_amd import _lib
    from tests.task_shaping_checks import record_rows
    return record_rows(env.get_task_inputs(), _lib.TASK_INPUT_FIELDS, _lib.TASK_INPUT_DIM)


def test_emulated_step_record_matches_the_oracle_and_the_fused_terms():
    """jvrc_step on the emulated stepper, both exports on, every walk mode in the batch: per control step the exported sites, targets,
    target state and root quaternion are the oracle's, the exported goal is the observation's goal block bit for bit, and
    VectorSteppingTask on the exported records gives the kernel's fused terms and termination.  (delay_frames shortened to 3, in kernel
    and oracle alike, so that targets advance within a few control steps.)"""
    from learninghumanoidwalking_amd import _lib
    from learninghumanoidwalking_amd.envs.jvrc_step import JvrcStepSpec
    from learninghumanoidwalking_amd.task_hook import VectorSteppingTask
    from oracle.env_jvrc_step import OracleJvrcStepEnv
    from tests import emu
    spec = JvrcStepSpec()
    spec.delay_frames = 3
    N, T = 7, 6
    env = emu.make_emulated(spec, N, seed=7)
    orc = [OracleJvrcStepEnv(spec, seed=7, env_id=i) for i in range(N)]
    env.reset()
    for o in orc:
        o.reset()
    assert {o.mode for o in orc} == {0, 1, 2, 3, 4}
    env.enable_task_inputs(True)
    env.enable_step_task_inputs()
    task = VectorSteppingTask(spec, "cpu")
    tape = (np.random.default_rng(3).normal(size=(T, N, 12)) * 0.1).astype(np.float32)
    advanced = 0
    for t in range(T):
        obs, rew, done, _ = env.step(tape[t])
        for i, o in enumerate(orc):
            o.step(tape[t, i])
        srec = _step_record(env)
        s = _lib.split_step_task_inputs(srec)
        for i, o in enumerate(orc):
            np.testing.assert_allclose(s["lsite_xpos"][i], o.l_foot_pos, rtol=0, atol=1e-12, err_msg=f"t={t} env={i}")
            np.testing.assert_allclose(s["rsite_xpos"][i], o.r_foot_pos, rtol=0, atol=1e-12, err_msg=f"t={t} env={i}")
            np.testing.assert_allclose(s["target1"][i], o.sequence[o.t1][:4], rtol=0, atol=1e-12)
            np.testing.assert_allclose(s["target2"][i], o.sequence[o.t2][:4], rtol=0, atol=1e-12)
            assert [s["t1"][i], s["t2"][i], s["reached"][i], s["frames"][i], s["nseq"][i]] == \
                [o.t1, o.t2, int(o.target_reached), o.target_reached_frames, o.nseq], f"t={t} env={i}"
            np.testing.assert_allclose(s["root_xquat"][i], o.sim.xquat[o.root], rtol=0, atol=1e-12)
            advanced += o.t1 > 0 and t == T - 1
        np.testing.assert_array_equal(s["goal"].astype(np.float32), obs[:, 31:39])
        assert not srec[:, 31].any()
        ti = _records(_task_record(env), srec)
        r, d = task.evaluate(ti)
        mine = np.stack([task.last_terms[k].numpy() for k in task.TERMS], axis=1)
        # (rew_terms / rew are float32 roundings of the kernel's float64 values)
        np.testing.assert_allclose(env.rew_terms, mine, rtol=0, atol=1e-7, err_msg=f"terms t={t}")
        np.testing.assert_allclose(rew, r.numpy(), rtol=0, atol=2e-7)
        np.testing.assert_array_equal(done & 1, d.numpy().astype(np.uint8), err_msg=f"done t={t}")
        if t % 3 == 2:       # resynchronise the chaotic dynamics (as the stepper's oracle tests do)
            q = np.array([o.sim.qpos for o in orc]); v = np.array([o.sim.qvel for o in orc])
            env.set_state(q, v)
            for o in orc:
                o.set_state(o.sim.qpos.copy(), o.sim.qvel.copy())
    assert advanced > 0


def test_emulated_resident_step_record_equals_the_per_step_record(monkeypatch):
    """lhw_env_rollout_step_task_inputs: the [T][N][32] stepping record of one launch equals, control step by control step, what
    lhw_env_get_step_task_inputs returns behind each step of the launch-per-step pipeline -- across truncations / auto-resets, and
    through the job-queue kernel (LHW_ROLLOUT_SLOTS / LHW_ROLLOUT_CHUNK)."""
    from learninghumanoidwalking_amd import _lib
    from learninghumanoidwalking_amd.envs.jvrc_step import JvrcStepSpec
    from tests import emu
    from tests.test_rollout_resident import NumpyActor, _buffers, _same
    spec = JvrcStepSpec()
    N, T = 4, 7
    envs = [emu.make_emulated(spec, N, seed=3, max_traj_len=4) for _ in range(3)]
    pol = NumpyActor(spec.obs_dim, spec.act_dim, seed=5, scale=2.0)
    obs0 = [e.reset().copy() for e in envs]
    L = emu.lib()
    envs[0].enable_task_inputs(True)
    envs[0].enable_step_task_inputs()
    a = _buffers(T, N, spec.obs_dim, spec.act_dim)
    a["obs"][0] = obs0[0]
    want = np.zeros((T, N, _lib.STEP_TASK_INPUT_DIM))
    want_tin = np.zeros((T, N, _lib.TASK_INPUT_DIM))
    y = np.zeros((N, pol.view.act_pad), np.float32)
    for t in range(T):
        assert L.lhw_debug_policy_step(ctypes.byref(pol.view), a["obs"][t].ctypes.data, N, 0, pol.view.counter + t, y.ctypes.data,
                                       a["act"][t].ctypes.data, a["logp"][t].ctypes.data, None) == 0
        obs, rew, done, tob = envs[0].step(a["act"][t])
        a["obs"][t + 1], a["rew"][t], a["done"][t], a["tob"][t] = obs, rew, done, tob
        want[t] = _step_record(envs[0])
        want_tin[t] = _task_record(envs[0])
    assert (a["done"] & 2).any()

    def resident(env, o0):
        b = _buffers(T, N, spec.obs_dim, spec.act_dim)
        b["obs"][0] = o0
        tin = np.full((T, N, _lib.TASK_INPUT_DIM), np.nan)
        stin = np.full((T, N, _lib.STEP_TASK_INPUT_DIM), np.nan)
        assert env.rollout(pol.view, T, b["obs"], b["act"], b["logp"], b["tob"], b["rew"], b["done"], task_inputs=tin, step_task_inputs=stin)
        return b, tin, stin

    monkeypatch.setenv("LHW_ROLLOUT_CHUNK", "0")
    b, tin, stin = resident(envs[1], obs0[1])
    assert not envs[1].last_rollout_queued()
    monkeypatch.setenv("LHW_ROLLOUT_CHUNK", "3")
    monkeypatch.setenv("LHW_ROLLOUT_SLOTS", "1")
    c, tin_q, stin_q = resident(envs[2], obs0[2])
    assert envs[2].last_rollout_queued()
    used = np.zeros(_lib.TASK_INPUT_DIM, bool)
    for o, n in _lib.TASK_INPUT_FIELDS.values():
        used[o:o + n] = True
    for buf, ti, st in ((b, tin, stin), (c, tin_q, stin_q)):
        _same(a, buf)
        np.testing.assert_array_equal(st, want)
        np.testing.assert_array_equal(ti[:, :, used], want_tin[:, :, used])
    # the API refuses the stepping record on other tasks and without the first record
    from learninghumanoidwalking_amd.envs.jvrc_walk import JvrcWalkSpec
    walk = emu.make_emulated(JvrcWalkSpec(), 2, seed=1)
    assert walk._L.lhw_env_enable_step_task_inputs(walk._h, 1) == -4
    assert L.lhw_env_rollout_step_task_inputs(envs[1]._h, ctypes.byref(pol.view), 0, N, T, *([None] * 8), stin.ctypes.data, None) == -1


def test_step_task_input_fields_equal_the_header():
    from learninghumanoidwalking_amd import _lib
    src = open(os.path.join(ROOT, "include", "lhw.h")).read()
    body = re.search(r"enum LhwStepTaskInput \{(.*?)\};", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    vals = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"LHW_STIN_(\w+)\s*=\s*(\d+)", body)}
    dim = int(re.search(r"LHW_STEP_TASK_INPUT_DIM\s*=\s*(\d+)", body).group(1))
    assert dim == _lib.STEP_TASK_INPUT_DIM == 32
    assert vals == {k: o for k, (o, _) in _lib.STEP_TASK_INPUT_FIELDS.items()}
    ends = sorted((o, o + n) for o, n in _lib.STEP_TASK_INPUT_FIELDS.values())
    assert all(a[1] == b[0] for a, b in zip(ends, ends[1:])) and ends[0][0] == 0 and ends[-1][1] == dim - 1     # contiguous, 31 reserved


def test_stepping_fields_need_the_stepping_record():
    from learninghumanoidwalking_amd import _lib
    from learninghumanoidwalking_amd.task_hook import TaskInputs
    ti = TaskInputs(torch.zeros(3, _lib.TASK_INPUT_DIM, dtype=torch.float64), 19, 18, 12)
    assert ti.grf_r.shape == (3,)
    with pytest.raises(AttributeError, match="stepping task"):
        ti.target1
    with pytest.raises(AttributeError):
        ti.no_such_field
    ti = _records(np.zeros((3, _lib.TASK_INPUT_DIM)), np.arange(96, dtype=np.float64).reshape(3, 32))
    assert ti.target1.shape == (3, 4) and ti.target1[1, 0] == 32 + 6 and ti.reached[2] == 64 + 14
    assert set(_lib.STEP_TASK_INPUT_FIELDS) <= set(ti.numpy())


def test_reward_only_is_honoured_only_on_the_env_whose_termination_the_task_declares():
    from learninghumanoidwalking_amd import batched_env as be
    from learninghumanoidwalking_amd.envs.h1 import H1Spec
    from learninghumanoidwalking_amd.envs.h1_walk import H1WalkSpec
    from learninghumanoidwalking_amd.envs.jvrc_step import JvrcStepSpec
    from learninghumanoidwalking_amd.envs.jvrc_walk import JvrcWalkSpec
    from learninghumanoidwalking_amd.task_hook import (VectorStandingTask, VectorSteppingTask, VectorTask, VectorWalkingTask,
                                                       reward_only_on)
    walk, stand, step = VectorWalkingTask(JvrcWalkSpec(), "cpu"), VectorStandingTask(H1Spec(), "cpu"), VectorSteppingTask(JvrcStepSpec(), "cpu")
    assert JvrcWalkSpec.task_code == be.TASK_JVRC_WALK and H1WalkSpec.task_code == be.TASK_H1_WALK
    assert H1Spec.task_code == be.TASK_H1_STAND and JvrcStepSpec.task_code == be.TASK_JVRC_STEP
    # a task on another env than the one whose fused termination its done() restates: consulted step by step
    assert not reward_only_on(walk, be.TASK_JVRC_STEP)
    assert not reward_only_on(step, be.TASK_JVRC_WALK)
    assert not reward_only_on(stand, be.TASK_H1_WALK)
    # each shipped task on its own env(s)
    for task, spec in ((walk, JvrcWalkSpec), (walk, H1WalkSpec), (stand, H1Spec), (step, JvrcStepSpec)):
        assert reward_only_on(task, spec.task_code)
    # another termination rule than the fused one
    assert not reward_only_on(VectorSteppingTask(JvrcStepSpec(), "cpu", min_root_height=0.6000001), be.TASK_JVRC_STEP)
    assert reward_only_on(VectorSteppingTask(JvrcStepSpec(), "cpu", weights=dict(step_reward=0.9)), be.TASK_JVRC_STEP)
    with pytest.raises(KeyError):
        VectorSteppingTask(JvrcStepSpec(), "cpu", weights=dict(no_such_term=1.0))

    # an undeclared user task: taken at its word, on any env, as before
    class Mine(VectorTask):
        reward_only = True
    assert reward_only_on(Mine(), be.TASK_JVRC_STEP) and reward_only_on(Mine(), be.TASK_JVRC_WALK)
    assert not reward_only_on(VectorTask(), be.TASK_JVRC_WALK) and not reward_only_on(None, be.TASK_JVRC_WALK)
    # Rollout decides with the same predicate (a host-only stand-in env: nothing is launched by the constructor)
    from learninghumanoidwalking_amd.ppo import Rollout
    env = SimpleNamespace(n_envs=2, obs_dim=39, act_dim=12, device=torch.device("cpu"), task=be.TASK_JVRC_STEP, history_len=1)
    assert not Rollout(env, None, 4, task=walk).reward_only
    assert Rollout(env, None, 4, task=step).reward_only
    assert Rollout(env, None, 4, task=Mine()).reward_only
