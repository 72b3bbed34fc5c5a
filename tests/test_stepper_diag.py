"""The diagnostic clocks of the humanoid steppers on the SIMT emulator (lhw_env_phase_cycles, lhw_env_debug_wave_cycles; include/lhw.h): the
kernels that carry them (control_step<.., DIAG>) are instantiations of their own, launched while a clock is armed.  Both variants are
compiled into the emulated library; arming must not change a stored value, and the armed kernels must record.  CPU twin of
tests/test_stepper_diag_gpu.py::test_armed_clocks_change_no_stored_bit_and_record (the emulator's shader clock ticks once per read)."""
import functools

import numpy as np
import pytest

from tests import emu
from tests.test_rollout_resident import NumpyActor, _per_step, _resident, _same

N, T = 5, 6      # odd: the last wavefront of the two-envs-per-wave kernels holds one env; jvrc_step runs one env per wave


def _spec(name):
    if name == "jvrc_walk":
        from learninghumanoidwalking_amd.envs.jvrc_walk import JvrcWalkSpec as S
    else:
        from learninghumanoidwalking_amd.envs.jvrc_step import JvrcStepSpec as S
    return S()


def _run(name, resident, armed):
    spec = _spec(name)
    env = emu.make_emulated(spec, N, seed=3, max_traj_len=4)      # truncation + auto-reset inside the rollout
    phase, wave = np.zeros(16, np.int64), np.zeros(N, np.int64)
    if armed:
        env.phase_cycles()
        env.wave_cycles()      # (the first call arms)
    pol = NumpyActor(spec.obs_dim, spec.act_dim, seed=5, scale=2.0)
    obs0 = env.reset().copy()
    b = (_resident if resident else _per_step)(env, pol, T, obs0)
    if armed:
        phase, wave = env.phase_cycles(), env.wave_cycles()
    state = env.get_state()
    env.close()
    return b, state, phase, wave


@functools.lru_cache(maxsize=None)
def _reference(name):
    """launch per step, no clock armed: computed once per env"""
    b, state, _, _ = _run(name, False, False)
    return b, state


@pytest.mark.parametrize("resident,armed", [(True, False), (False, True), (True, True)])
@pytest.mark.parametrize("name", ["jvrc_walk", "jvrc_step"])
def test_armed_clocks_change_no_stored_bit_and_record(name, resident, armed):
    ref, ref_state = _reference(name)
    b, state, phase, wave = _run(name, resident, armed)
    _same(ref, b)
    for x, y in zip(ref_state, state):
        np.testing.assert_array_equal(x, y)
    if armed:      # slot 0 kinematics, 3 collision, 7 Newton (cycles of env 0), 6 its Newton passes
        assert phase[0] > 0 and phase[3] > 0 and phase[7] > 0 and phase[6] > 0, phase
        assert (wave > 0).all(), wave
    else:
        assert not phase.any() and not wave.any()
