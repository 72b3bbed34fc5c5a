"""Host-side task specs and the oracle's task layer against fixtures generated from the reference (CPU)."""
import os
import subprocess
import sys

import numpy as np

from learninghumanoidwalking_amd.envs.jvrc_walk import JvrcWalkSpec, phase_clock_lut

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_clock_lut_is_bit_exact_with_reference_pchip():
    g = np.load(os.path.join(G, "rewards.npz"))
    spec = JvrcWalkSpec()
    assert spec.period == 88 and spec.frame_skip == 25
    np.testing.assert_array_equal(spec.clock_lut(), g["jvrc_lut"])
    np.testing.assert_array_equal(phase_clock_lut(0.4, 0.1, 0.1, 40, 40), g["h1_lut"])
    lut = spec.clock_lut()
    dbl = [p for p in range(88) if lut[0, p] == 1 and lut[2, p] == 1]
    assert dbl == list(range(32, 43)) + list(range(76, 87))      # SURVEY.md 8c known answer


def test_mirror_tables_equal_reference_matrices():
    g = np.load(os.path.join(G, "misc.npz"))
    (osrc, osign), (asrc, asign) = JvrcWalkSpec().mirror_tables()
    x = np.random.default_rng(0).normal(size=(4, 37))
    ref = x @ g["mir_obs"]
    ref[:, [29, 30]] *= -1            # clock entries: sin(arcsin(c) + pi) == -c
    np.testing.assert_allclose(x[:, osrc] * osign, ref, atol=0)
    a = np.random.default_rng(1).normal(size=(4, 12))
    np.testing.assert_allclose(a[:, asrc] * asign, a @ g["mir_act"], atol=0)


def test_mirror_tables_of_h1_walk_and_jvrc_step_equal_reference_matrices():
    from learninghumanoidwalking_amd.envs import H1WalkSpec, JvrcStepSpec
    g = np.load(os.path.join(G, "misc.npz"))
    for spec, D, A, mo, ma, clock in ((H1WalkSpec(), 43, 10, g["mir_obs_h1walk"], g["mir_act_h1walk"], [35, 36]),
                                      (JvrcStepSpec(), 39, 12, g["mir_obs_step"], g["mir_act"], [29, 30])):
        (osrc, osign), (asrc, asign) = spec.mirror_tables()
        x = np.random.default_rng(0).normal(size=(4, D))
        ref = x @ mo
        ref[:, clock] *= -1
        np.testing.assert_allclose(x[:, osrc] * osign, ref, atol=0)
        a = np.random.default_rng(1).normal(size=(4, A))
        np.testing.assert_allclose(a[:, asrc] * asign, a @ ma, atol=0)
        assert spec.mirror_inds()[2] == clock and spec.obs_mean.shape == (D,) and spec.obs_std.shape == (D,)


def test_h1_walk_clock_matches_reference_spline_table():
    from learninghumanoidwalking_amd.envs import H1WalkSpec
    g = np.load(os.path.join(G, "rewards.npz"))
    s = H1WalkSpec()
    assert s.period == 40
    np.testing.assert_allclose(s.clock_lut(), g["h1_lut"], rtol=0, atol=1e-15)


def test_oracle_reward_terms_equal_reference_functions():
    from oracle import env_jvrc_walk as e
    g = np.load(os.path.join(G, "rewards.npz"))
    i = g["inputs"]
    qvel, qacc, tq, ptq, a, pa = i[:18], i[18:36], i[36:48], i[48:60], i[60:72], i[72:84]
    mine = np.array([
        e.r_fwd_vel(np.array([0.3, -0.1]), np.array([0.2, 0.0])), e.r_yaw_vel(0.37, 0.1), e.r_action(a, pa), e.r_torque(tq, ptq),
        e.r_height(0.77, 0.8, 0.2, 0.005), e.r_height(0.795, 0.8, 0.0, 0.0), e.r_root_accel(qvel, qacc),
        e.r_clock(120.0, 500.0, -1.0, 0.5, 62.0 * 9.8 * 0.5),
        e.r_clock(np.linalg.norm([0.1, 0, 0.05]), np.linalg.norm([0.3, 0.1, 0]), 1.0, -0.25, 0.2)])
    np.testing.assert_allclose(mine, g["terms"], rtol=0, atol=1e-15)


def test_oracle_env_surface_like_reference_tests():
    """Shape / finiteness / reward-sum checks of reference tests/test_environments.py:39-188 on the oracle env."""
    from oracle.env_jvrc_walk import make_oracle_jvrc_walk
    env = make_oracle_jvrc_walk(seed=3)
    obs = env.reset()
    assert obs.shape == (37,) and np.isfinite(obs).all()
    rs = np.random.default_rng(0)
    for _ in range(20):
        obs, r, done, info = env.step(rs.normal(size=12) * 0.2)
        assert obs.shape == (37,) and np.isfinite(obs).all() and isinstance(done, bool)
        assert abs(r - sum(info.values())) < 1e-6 and len(info) == 10
        if done:
            env.reset()


def test_device_rng_header_matches_python_restatement(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include "%s/learninghumanoidwalking_amd/csrc/lhw_rng.h"\nint main(){'
                   'for(unsigned e=0;e<3;e++)for(unsigned c=0;c<3;c++)for(unsigned s=0;s<3;s++)'
                   'printf("%%llu %%.17g %%d\\n",(unsigned long long)lhw_rng_bits(12345ull,e,2,c*1000+7,s),'
                   'lhw_rng_uniform(12345ull,e,1,c,s,-0.5,0.5),lhw_rng_randint(99ull,e,2,c,s,88));return 0;}' % ROOT)
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-O1", "-o", str(exe), str(src), "-lm"])
    out = subprocess.check_output([str(exe)]).decode().split("\n")
    from oracle import rng
    k = 0
    for e in range(3):
        for c in range(3):
            for s in range(3):
                b, u, r = out[k].split()
                assert int(b) == rng.bits(12345, e, 2, c * 1000 + 7, s)
                assert float(u) == rng.uniform(12345, e, 1, c, s, -0.5, 0.5)
                assert int(r) == rng.randint(99, e, 2, c, s, 88)
                k += 1


def test_jvrc_yaml_keys_of_base_humanoid_env_follow_the_reference_key_by_key(tmp_path):
    """BaseHumanoidEnv's generic hooks on a JVRC env, as the reference's code treats them (envs/common/base_humanoid_env.py:76-92,
    247-338; envs/jvrc/jvrc_base.py:133-138; envs/common/domain_randomization.py:44): observation_noise is never applied by the JVRC
    robot state -> accepted and ignored; dynamics_randomization fails there (no body named 'pelvis') -> refused; init_noise and perturbation
    run there and here."""
    import pytest
    import yaml
    from learninghumanoidwalking_amd.envs.jvrc_walk import JVRC_BASE_YAML
    base = yaml.safe_load(open(JVRC_BASE_YAML))

    def spec_with(**extra):
        p = tmp_path / ("cfg_" + "_".join(extra) + ".yaml")
        p.write_text(yaml.safe_dump(dict(base, **extra)))
        return JvrcWalkSpec(yaml_path=str(p))

    s = spec_with(observation_noise=dict(enabled=True, type="uniform", multiplier=1.0, scales=dict(root_orient=0.05)))
    assert s.obs_dim == 37
    with pytest.raises(NotImplementedError):
        spec_with(dynamics_randomization=dict(enable=True, interval=0.5))
    with pytest.raises(NotImplementedError):
        spec_with(perturbation=dict(enable=True, interval=5.0, bodies=["PELVIS_S", "R_KNEE_S", "L_KNEE_S"]))      # more than two bodies
    assert spec_with(init_noise=3).init_noise_deg == 3.0
    sp = spec_with(perturbation=dict(enable=True, interval=5.0, bodies=["PELVIS_S"], force_magnitude=10, torque_magnitude=2))
    assert sp.perturb_interval == 200 and sp.perturbation_config()["force"] == 10.0
    assert spec_with(perturbation=dict(enable=False, interval=5.0, bodies=["PELVIS_S"])).perturbation_config() is None
    spec_with(dynamics_randomization=dict(enable=False, interval=0.5), init_noise=0)      # configured but off: fine


def test_env_args_of_every_spec_needs_no_torch():
    """what a spec hands to the kernels is host arithmetic: it must be computable where torch cannot even be imported"""
    code = ("import sys; sys.modules['torch'] = None\n"
            "from learninghumanoidwalking_amd.envs import ENVIRONMENTS\n"
            "for name, cls in ENVIRONMENTS.items():\n"
            "    model, task, kw = cls().env_args()\n"
            "    assert task == cls.task_code and kw['frame_skip'] > 0, name\n"
            "assert sys.modules['torch'] is None\n"
            "print('ok', len(ENVIRONMENTS))\n")
    out = subprocess.check_output([sys.executable, "-c", code], cwd=ROOT).decode()
    assert out.split() == ["ok", "5"]


def test_env_args_contents():
    import inspect
    from learninghumanoidwalking_amd import _lib
    from learninghumanoidwalking_amd.envs import ENVIRONMENTS
    accepted = set(inspect.signature(_lib.env_config).parameters) | {"history_len"}
    per_call = {"n_envs", "seed", "device", "max_traj_len", "env_id_base"}
    codes = dict(cartpole=_lib.TASK_CARTPOLE, jvrc_walk=_lib.TASK_JVRC_WALK, jvrc_step=_lib.TASK_JVRC_STEP, h1=_lib.TASK_H1_STAND,
                 h1_walk=_lib.TASK_H1_WALK)
    for name, cls in ENVIRONMENTS.items():
        spec = cls()
        model, task, kw = spec.env_args()
        assert task == spec.task_code == codes[name]
        assert set(kw) <= accepted and not set(kw) & per_call, name
        assert kw["frame_skip"] == spec.frame_skip
        if name == "cartpole":
            assert kw.get("clock_lut") is None and kw.get("nominal_qpos") is None
            continue
        assert len(kw["nominal_qpos"]) == model.nq and len(kw["action_offset"]) == len(kw["kp"]) == len(kw["kd"]) == spec.act_dim
        assert kw["history_len"] == 1
        if name == "h1":
            assert kw["clock_lut"] is None
        else:
            assert np.asarray(kw["clock_lut"]).shape == (4, spec.period)
        # the two encodings of init noise / perturbation: H1 through the task parameters, JVRC through the config record
        assert ("init_noise" in kw and "perturbation" in kw) == name.startswith("jvrc")


def test_emulated_env_built_from_env_args_steps_jvrc_walk():
    from tests import emu
    spec = JvrcWalkSpec()
    model, task, kw = spec.env_args()
    env = emu.EmuBatchedEnv(model, task, 2, seed=3, **kw)
    obs = env.reset().copy()
    assert obs.shape == (2, 37) and np.isfinite(obs).all()
    obs2, rew, done, _ = env.step(np.zeros((2, 12), np.float32))
    assert np.isfinite(obs2).all() and np.isfinite(rew).all() and not np.array_equal(obs, obs2)
    assert env.pop_fault_stats() == (0, 0)
    env.close()


def test_config_filler_refuses_three_perturbation_bodies():
    import pytest
    from learninghumanoidwalking_amd import _lib
    from tests import emu
    model, task, kw = JvrcWalkSpec().env_args()
    three = dict(interval=200, bodies=[1, 2, 3], force=10.0, torque=2.0)
    with pytest.raises(ValueError, match="at most two bodies"):
        _lib.env_config(task, 1, **dict({k: v for k, v in kw.items() if k != "history_len"}, perturbation=three))
    with pytest.raises(ValueError, match="at most two bodies"):      # the emulated env goes through the same filler
        emu.EmuBatchedEnv(model, task, 1, **dict(kw, perturbation=three))
    cfg, keep = _lib.env_config(task, 1, **dict({k: v for k, v in kw.items() if k != "history_len"}, perturbation=dict(three, bodies=[1, 2])))
    assert (cfg.perturb_interval, cfg.n_perturb_bodies, list(cfg.perturb_bodies), cfg.perturb_force) == (200, 2, [1, 2], 10.0)
    assert cfg.period == 88 and cfg.n_task_params == 1 and cfg.n_task_iparams == 4 and len(keep) == 7


def test_control_dt_must_be_a_multiple_of_sim_dt_for_both_robots(tmp_path):
    """robots/robot_base.py:37-38, constructed by H1BaseEnv (h1_base.py:64) and by JvrcBaseEnv (jvrc_base.py:63) alike"""
    import pytest
    import yaml
    from learninghumanoidwalking_amd.envs import H1Spec
    from learninghumanoidwalking_amd.envs.h1 import H1_BASE_YAML, load_config
    from learninghumanoidwalking_amd.envs.jvrc_walk import JVRC_BASE_YAML
    for cls, base in ((H1Spec, load_config(H1_BASE_YAML)), (JvrcWalkSpec, yaml.safe_load(open(JVRC_BASE_YAML)))):
        p = tmp_path / (cls.name + ".yaml")
        p.write_text(yaml.safe_dump(dict(base, sim_dt=0.001, control_dt=0.0255)))
        spec = cls(yaml_path=str(p))
        with pytest.raises(Exception, match="integer multiple"):
            spec.frame_skip
        with pytest.raises(Exception, match="integer multiple"):
            spec.env_args()
        assert cls().frame_skip == 25


def test_make_batched_builds_the_substitutable_env_class_from_env_args(monkeypatch):
    """envs.humanoid.BatchedEnv is the seam an emulated backend or a recorder replaces: make_batched hands it env_args() plus the
    per-call arguments, for every spec"""
    from learninghumanoidwalking_amd.envs import ENVIRONMENTS, humanoid
    got = {}

    class Recorder:
        def __init__(self, model, task, n_envs, **kw):
            got.update(model=model, task=task, n_envs=n_envs, kw=kw)

    assert humanoid.BatchedEnv is None          # (the GPU class is looked up at call time: importing a spec needs no torch)
    monkeypatch.setattr(humanoid, "BatchedEnv", Recorder)
    for name, cls in ENVIRONMENTS.items():
        spec = cls()
        env = spec.make_batched(3, seed=5, max_traj_len=7, env_id_base=11)
        model, task, kw = spec.env_args()
        assert isinstance(env, Recorder) and (got["task"], got["n_envs"]) == (task, 3), name
        for a, b in zip(got["model"].pack(), model.pack()):
            np.testing.assert_array_equal(a, b)
        assert set(got["kw"]) == set(kw) | {"seed", "device", "max_traj_len", "env_id_base"}
        assert (got["kw"]["seed"], got["kw"]["device"], got["kw"]["max_traj_len"], got["kw"]["env_id_base"]) == (5, 0, 7, 11)
