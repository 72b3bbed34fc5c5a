"""The diagnostic clocks of the humanoid steppers on the GPU (lhw_env_phase_cycles, lhw_env_debug_wave_cycles; include/lhw.h): they live in
kernels of their own (control_step<.., DIAG>: humanoid_diag_kernel, humanoid_rollout_diag_kernel), launched while a clock is armed.  Arming
must not change a stored bit, the armed kernels must record -- launch per step, resident, through the job queue --, and what has no kernels
with clocks (term statistics, observation history) must behave as include/lhw.h says instead of recording nothing.  In the same file: the
task parameters sit behind the model record in ONE device block now (HDevBlock), and lhw_env_set_task_shaping writes through it.
CPU twin of the first test: tests/test_stepper_diag.py (SIMT emulator)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, T = 5, 6      # odd: the last wavefront of the two-envs-per-wave kernels holds one env; jvrc_step runs one env per wave
NAMES = ("obs", "act", "logp", "tob_all", "rew", "done", "val", "vterm", "vfinal")


def _args(n, t, std=0.4):
    return SimpleNamespace(gamma=0.99, lam=0.95, lr=3e-4, eps=1e-5, entropy_coeff=0.0, clip=0.2, minibatch_size=n * t, epochs=1,
                           max_traj_len=t, num_procs=n, num_envs=n, max_grad_norm=0.5, mirror_coeff=0.4, eval_freq=10**9,
                           recurrent=False, imitate=None, learn_std=False, std_dev=std, no_mirror=True, continued=None,
                           logdir="/tmp/lhw_test_diag", device_index=0)


def _buffers(ro):
    return [getattr(ro, n).clone() for n in NAMES]


def _arm(env):
    env.phase_cycles(True)      # arms the phase clock (and reads zeros)
    env.wave_cycles()           # the first call arms the wave clock


def _run(env_name, mode, armed, monkeypatch, queue=False):
    """one rollout of N envs x T steps through PPO's collector; (buffers, state, phase cycles or None, wave cycles or None, queued)"""
    from learninghumanoidwalking_amd.envs import ENVIRONMENTS
    from learninghumanoidwalking_amd.ppo import PPO
    monkeypatch.setenv("LHW_ROLLOUT_MODE", mode)
    if queue:
        monkeypatch.setenv("LHW_ROLLOUT_SLOTS", "2")
        monkeypatch.setenv("LHW_ROLLOUT_CHUNK", "2")
    else:
        monkeypatch.delenv("LHW_ROLLOUT_SLOTS", raising=False)
        monkeypatch.delenv("LHW_ROLLOUT_CHUNK", raising=False)
    algo = PPO(ENVIRONMENTS[env_name], _args(N, T), seed=9, term_stats=False)
    if armed:
        _arm(algo.env)
    algo.sample_parallel_with_workers()
    assert algo.rollout.last_mode == mode
    phase = algo.env.phase_cycles(True) if armed else None
    wave = algo.env.wave_cycles() if armed else None
    return _buffers(algo.rollout), algo.env.get_state(), phase, wave, algo.env.last_rollout_queued()


@functools.lru_cache(maxsize=None)
def _reference(env_name):
    """the launch-per-step rollout with no clock armed: computed once per env, compared against by every case below"""
    mp = pytest.MonkeyPatch()
    try:
        buf, state, _, _, _ = _run(env_name, "steps", False, mp)
    finally:
        mp.undo()
    return buf, state


def _same(ref, buf, state):
    for n, x, y in zip(NAMES, ref[0], buf):
        assert torch.equal(x, y), n
    for x, y in zip(ref[1], state):
        np.testing.assert_array_equal(x, y)


def _recorded(phase, wave):
    # include/lhw.h: slot 0 kinematics, 3 collision, 7 Newton (cycles of env 0); 6 counts its Newton passes
    print("phase cycles", phase.tolist(), "wave cycles", wave.tolist())
    assert phase[0] > 0 and phase[3] > 0 and phase[7] > 0 and phase[6] > 0
    assert wave.shape == (N,) and (wave > 0).all()


@pytest.mark.parametrize("mode,armed", [("resident", False), ("steps", True), ("resident", True)])
@pytest.mark.parametrize("env_name", ["jvrc_walk", "jvrc_step"])
def test_armed_clocks_change_no_stored_bit_and_record(env_name, mode, armed, monkeypatch):
    buf, state, phase, wave, queued = _run(env_name, mode, armed, monkeypatch)
    assert not queued
    _same(_reference(env_name), buf, state)
    if armed:
        _recorded(phase, wave)


def test_a_queued_rollout_records_as_well(monkeypatch):
    """stepping task, more env groups (5) than wave slots (2): the resident waves drain the job queue in chunks of 2 control steps, and a
    group's wave clock is the sum over its chunks"""
    buf, state, phase, wave, queued = _run("jvrc_step", "resident", True, monkeypatch, queue=True)
    assert queued
    _same(_reference("jvrc_step"), buf, state)
    _recorded(phase, wave)


def test_term_statistics_and_the_clocks_exclude_each_other(monkeypatch):
    """the kernels that keep the term statistics carry no clocks: whichever of the two comes second is refused with LHW_ERR_UNSUPPORTED
    (-4) and changes nothing -- the env goes on as it was armed first"""
    from learninghumanoidwalking_amd import _lib
    from learninghumanoidwalking_amd.envs import ENVIRONMENTS
    from learninghumanoidwalking_amd.ppo import PPO
    monkeypatch.setenv("LHW_ROLLOUT_MODE", "resident")
    # statistics first: neither clock can be armed, the statistics kernels go on running resident
    algo = PPO(ENVIRONMENTS["jvrc_walk"], _args(N, T), seed=9, term_stats=True)
    for arm in (lambda: algo.env.phase_cycles(True), algo.env.wave_cycles):
        with pytest.raises(_lib.LhwError) as e:
            arm()
        assert e.value.code == -4 and "term statistics" in str(e.value)
    algo.sample_parallel_with_workers()
    assert algo.rollout.last_mode == "resident" and algo.term_stats is not None
    _same(_reference("jvrc_walk"), _buffers(algo.rollout), algo.env.get_state())
    assert not algo.env.phase_cycles(False).any()      # (reading without arming: nothing was recorded, nothing is armed)
    # a clock first: the statistics cannot be switched on, the clock goes on recording
    algo = PPO(ENVIRONMENTS["jvrc_walk"], _args(N, T), seed=9, term_stats=False)
    _arm(algo.env)
    with pytest.raises(_lib.LhwError) as e:
        algo.env.enable_term_stats(True)
    assert e.value.code == -4 and "clock" in str(e.value)
    algo.sample_parallel_with_workers()
    assert algo.rollout.last_mode == "resident"
    _same(_reference("jvrc_walk"), _buffers(algo.rollout), algo.env.get_state())
    _recorded(algo.env.phase_cycles(True), algo.env.wave_cycles())


def test_a_history_rollout_with_an_armed_clock_is_declined_and_the_steps_record(tmp_path, monkeypatch):
    """obs_history_len = 2: the history family has no kernels with clocks, so with a clock armed lhw_env_rollout_history declines
    (LHW_ERR_UNSUPPORTED: BatchedEnv.rollout returns False) and the collector steps launch by launch -- the same bits as the resident
    rollout of an env with no clock armed, and the clocks have run"""
    from learninghumanoidwalking_amd import _lib
    from tests.test_rollout_history_gpu import _ppo

    def run(mode, armed):
        monkeypatch.setenv("LHW_ROLLOUT_MODE", mode)
        algo = _ppo(tmp_path, "jvrc_walk", 2, N, T, seed=9)
        if armed:
            _arm(algo.env)
        return algo

    plain = run("auto", False)
    plain.sample_parallel_with_workers()
    assert plain.rollout.last_mode == "resident"
    armed = run("auto", True)
    armed.sample_parallel_with_workers()
    assert armed.rollout.last_mode == "steps"
    for n, x, y in zip(NAMES, _buffers(plain.rollout), _buffers(armed.rollout)):
        assert torch.equal(x, y), n
    _recorded(armed.env.phase_cycles(True), armed.env.wave_cycles())
    forced = run("resident", True)      # (LHW_ROLLOUT_MODE=resident turns a declined rollout into an error: the library's own message)
    with pytest.raises(_lib.LhwError) as e:
        forced.sample_parallel_with_workers()
    assert e.value.code == -4


def test_task_shaping_between_two_resident_rollouts_reaches_the_kernels(monkeypatch):
    """HParams sits at a fixed offset behind HModel in one device block: lhw_env_set_task_shaping between two resident rollouts must change
    the rewards of the second (and nothing else of it), and setting the default weights again must restore the bits of an unshaped run"""
    from learninghumanoidwalking_amd import _lib
    from learninghumanoidwalking_amd.envs import ENVIRONMENTS
    from learninghumanoidwalking_amd.ppo import PPO
    monkeypatch.setenv("LHW_ROLLOUT_MODE", "resident")

    def run(shape):
        algo = PPO(ENVIRONMENTS["jvrc_walk"], _args(N, T), seed=9, term_stats=False)
        out = []
        for k in range(3):
            if shape and k == 1:
                algo.env.set_task_shaping(reward_weights={"com_vel_error": 0.30, "yaw_vel_error": 0.10, "torque_penalty": 0.0, "action_penalty": 0.05})
            if shape and k == 2:
                algo.env.set_task_shaping(reward_weights=_lib.DEFAULT_REWARD_WEIGHTS[_lib.TASK_JVRC_WALK])
            algo.sample_parallel_with_workers()
            assert algo.rollout.last_mode == "resident"
            out.append(dict(zip(NAMES, _buffers(algo.rollout))))
        return out, algo.env.get_state()

    (a, sa), (b, sb) = run(False), run(True)
    for k in (0, 2):
        for n in NAMES:
            assert torch.equal(a[k][n], b[k][n]), (k, n)
    assert not torch.equal(a[1]["rew"], b[1]["rew"])
    for n in ("obs", "act", "logp", "tob_all", "done"):
        assert torch.equal(a[1][n], b[1][n]), n
    for x, y in zip(sa, sb):
        np.testing.assert_array_equal(x, y)
