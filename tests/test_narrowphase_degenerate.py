"""Degenerate branches of the primitive narrow phases of the HIP stepper against the CPU oracle, each entered on purpose and asserted --
from the oracle's geom poses, with the kernel's own deciding quantity -- to have been entered:

  * plane-cylinder with the axis along the plane normal (len_sqr < HMINVAL^2: the rim point is taken along the cylinder's x axis): the
    cylinder-shank variant of tests/cyl_variant.py with the shanks straightened and lengthened into stilts that reach below the feet, standing
    on the floor with identity orientation, 4e-16 rad off it (still below the threshold) and 3e-15 rad off it (just above);
  * sphere-cylinder with the sphere past a flat end, over the cap disk (a_sqr <= rad^2) and off the rim: the other leg's ankle ball under a
    stilt's end, in the air;
  * sphere-box with the sphere's centre inside the box (the sphere leaves through the nearest face): the unmasked variant of
    tests/test_primbox_parity.py, the left shin's sphere centred inside the right foot box, in the air;
  * capsule-capsule with parallel axes (|det| < HMINVAL: up to two contacts from the segment ends): the stand-in as shipped, in the air, both
    legs rolled the same way until the thigh capsules touch -- exactly parallel, 1e-9 rad off (still the parallel branch) and 1e-7 rad off
    (the general branch).  Within the joint ranges no two capsules of the stand-in can touch while parallel (the hips are 0.192 m apart,
    the radii add up to 0.1 m): the right hip roll is 0.75 rad past its limit, and its limit row is active.

Poses were found offline with the oracle.  Two control steps each, re-synchronised to the oracle after every step.  Runs on the SIMT
emulator in the CPU suite and on the GPU in the `-m gpu` suite."""
import numpy as np
import pytest

HMINVAL = 1e-15
# ---- stilts: root tilt about x for the standing envs, joint angles for the envs in the air (root at z = 1.3)
ROOT_Z_STANDING = 0.908                       # the stilts' lower caps 1 mm below the floor plane
TILTS = [0.0, 4e-16, 3e-15]
CAP = [
    [-1.3648, 0.0418, -0.2864, 2.0431, 0.245, -1.1647, -0.592, -0.2745, -0.341, 0.7635, 0.2536, 0.0286],
    [-0.4104, -0.0825, -0.3426, 0.9839, -0.1702, 0.2374, -0.8808, 0.0884, 0.3385, 1.6312, -0.4749, -0.1626],
]
RIM = [
    [-0.412, -0.0775, 0.0049, 0.2399, 0.2057, 0.0128, -1.2862, -0.2595, 0.4373, 1.6927, 0.0337, -0.2259],
    [-0.9327, 0.158, -0.0778, 2.2069, 0.1678, 0.1512, -1.0653, 0.6005, 0.3372, 2.4224, 0.5448, 0.0293],
]
# ---- unmasked variant: the left shin's sphere centred inside the right foot box
INSIDE = [
    [-0.6206, 0.1911, -0.2676, 1.8225, 0.1741, 0.3702, 0.2235, -0.0252, -0.4733, 0.4096, 0.0428, 0.6887],
    [-1.8044, 0.2358, -0.4274, 1.8509, -0.2447, -0.4246, -1.1624, 0.1878, -0.1386, 0.4018, 0.5883, -0.4442],
    [-1.6714, -0.462, -0.2629, 1.9745, -0.0546, -0.3602, -1.0447, -0.33, 0.0292, 0.9332, -0.5311, -0.6477],
]


# ---- the stand-in as shipped: both hip rolls, the left one off by 0 / 1e-9 / 1e-7 rad
PARALLEL_ROLL, PARALLEL_OFF = 1.1, [0.0, 1e-9, 1e-7]


def _stilt_spec(tmp_path):
    from learninghumanoidwalking_amd.envs.jvrc_walk import JvrcWalkSpec
    from tests.cyl_variant import cylinder_spec
    xml = open(cylinder_spec(tmp_path).xml_path).read()
    old = 'type="cylinder" size="0.045" fromto="0.01 0 -0.06 0.035 0 -0.28"'
    assert xml.count(old) == 2
    path = tmp_path / "jvrc_stilts.xml"
    path.write_text(xml.replace(old, 'type="cylinder" size="0.045 0.2" pos="0.02 0 -0.3"'))
    return JvrcWalkSpec(xml_path=str(path))


def _stilt_states(spec):
    n = len(TILTS) + len(CAP) + len(RIM)
    q = np.tile(np.array(spec.nominal_pose, float), (n, 1))
    q[:, 2] = 1.3
    q[:len(TILTS), 2] = ROOT_Z_STANDING
    q[:len(TILTS), 7:] = 0.0
    for i, th in enumerate(TILTS):
        q[i, 3:7] = [1.0, 0.5 * th, 0.0, 0.0]
    q[len(TILTS):, 7:] = CAP + RIM
    return q


def _contacts(m, sim, t1, t2):
    out = []
    for k in range(sim.ncon):
        c = sim.contact(k)
        if (int(m.geom_type[c["geom1"]]), int(m.geom_type[c["geom2"]])) == (t1, t2):
            out.append(c)
    return out


def _check_stilts(m, orc):
    """which side of the kernel's thresholds each env is on, from the oracle's geom poses (the operations of col_cylinder in
    csrc/lhw_humanoid_dev.h)"""
    for i, o in enumerate(orc):
        s = o.sim
        if i < len(TILTS):
            cons = _contacts(m, s, 0, 5)
            assert len(cons) == 6 and s.ncon == 6                     # three points per stilt, nothing else touches
            for g in {c["geom2"] for c in cons}:
                R = s.geom_xmat[g]
                axis, n = np.array([R[2], R[5], R[8]]), np.array([0.0, 0.0, 1.0])
                prj = n @ axis
                if prj > 0:
                    axis, prj = -axis, -prj
                vec = axis * prj - n
                len_sqr = vec @ vec
                if TILTS[i] == 0.0:
                    assert np.array_equal(R, np.eye(3).ravel()) and len_sqr == 0.0
                assert (len_sqr < HMINVAL * HMINVAL) == (i < 2), (i, len_sqr)
        else:
            cap = i < len(TILTS) + len(CAP)
            hit = 0
            for c in _contacts(m, s, 2, 5):
                R = s.geom_xmat[c["geom2"]]
                axis, vec = np.array([R[2], R[5], R[8]]), s.geom_xpos[c["geom1"]] - s.geom_xpos[c["geom2"]]
                rad, hl = m.geom_size[c["geom2"]][:2]
                x = vec @ axis
                a3 = vec - axis * x
                if abs(x) > hl and ((a3 @ a3 <= rad * rad) == cap) and abs(a3 @ a3 - rad * rad) > 1e-6:
                    hit += 1
            assert hit >= 1, (i, "cap" if cap else "rim")


def _check_inside(m, orc):
    names = list(m.geom_names)
    sph, box = names.index("L_KNEE_S-geom"), names.index("R_ANKLE_P_S-foot")
    for i, o in enumerate(orc):
        s = o.sim
        ctr = s.geom_xmat[box].reshape(3, 3).T @ (s.geom_xpos[sph] - s.geom_xpos[box])
        assert (np.abs(ctr) < m.geom_size[box] - 1e-4).all(), (i, ctr)              # centre inside the box, clear of every face
        assert any(c["geom1"] == sph and c["geom2"] == box for c in _contacts(m, s, 2, 6))


def _check_parallel(m, orc):
    names = list(m.geom_names)
    pair = (names.index("R_HIP_Y_S-geom"), names.index("L_HIP_Y_S-geom"))
    for i, o in enumerate(orc):
        s = o.sim
        a1, a2 = (s.geom_xmat[g].reshape(3, 3)[:, 2] for g in pair)
        ma, mb, mc = a1 @ a1, -(a1 @ a2), a2 @ a2
        det = ma * mc - mb * mb
        cons = [c for c in _contacts(m, s, 3, 3) if (c["geom1"], c["geom2"]) == pair]
        assert (abs(det) < HMINVAL) == (i < 2), (i, det)
        assert len(cons) == (2 if i < 2 else 1), (i, len(cons))


def _run(spec, q, check, env, orc, step, terms_of):
    m = spec.model()
    env.reset()
    for o in orc:
        o.reset()
    v = np.zeros((len(q), m.nv))
    env.set_state(q, v)
    for i, o in enumerate(orc):
        o.set_state(q[i], v[i])
    check(m, orc)                                                                    # the state the first sub-step collides
    act = (np.random.default_rng(26).normal(size=(2, len(q), 12)) * 0.1).astype(np.float32)
    for t in range(2):
        rew, done = step(act[t])
        res = [o.step(act[t, i]) for i, o in enumerate(orc)]
        gq, gv = env.get_state()
        oq = np.array([o.sim.qpos.copy() for o in orc]); ov = np.array([o.sim.qvel.copy() for o in orc])
        assert np.isfinite(oq).all() and np.abs(ov).max() < 50.0                     # the oracle itself is far from its NaN guard
        np.testing.assert_allclose(gq, oq, rtol=0, atol=1e-11, err_msg=f"qpos t={t}")
        np.testing.assert_allclose(gv, ov, rtol=0, atol=1e-8, err_msg=f"qvel t={t}")
        np.testing.assert_allclose(rew, np.array([r[1] for r in res]), rtol=0, atol=2e-6, err_msg=f"rew t={t}")
        terms = np.array([[r[3][k] for k in o.TERMS] for r, o in zip(res, orc)])
        np.testing.assert_allclose(terms_of(), terms, rtol=0, atol=2e-6, err_msg=f"terms t={t}")
        np.testing.assert_array_equal(done & 1, np.array([int(r[2]) for r in res], dtype=np.uint8), err_msg=f"done t={t}")
        env.set_state(oq, ov)
        for o in orc:
            o.set_state(o.sim.qpos.copy(), o.sim.qvel.copy())
    assert env.pop_fault_stats() == (0, 0)


def _case(tmp_path, name):
    if name == "stilts":
        spec = _stilt_spec(tmp_path)
        return spec, _stilt_states(spec), _check_stilts
    if name == "parallel_capsules":
        from learninghumanoidwalking_amd.envs.jvrc_walk import JvrcWalkSpec
        spec = JvrcWalkSpec()
        q = np.tile(np.array(spec.nominal_pose, float), (len(PARALLEL_OFF), 1))
        q[:, 2] = 1.3
        for i, off in enumerate(PARALLEL_OFF):
            q[i, 7:] = [-0.5, PARALLEL_ROLL, 0, 0.9, 0, -0.4, -0.5, PARALLEL_ROLL + off, 0, 0.9, 0, -0.4]
        return spec, q, _check_parallel
    from tests.test_primbox_parity import _spec
    spec = _spec(tmp_path)
    q = np.tile(np.array(spec.nominal_pose, float), (len(INSIDE), 1))
    q[:, 2] = 1.3
    q[:, 7:] = INSIDE
    return spec, q, _check_inside


def _oracles(spec, n):
    from oracle.env_jvrc_walk import OracleJvrcWalkEnv
    return [OracleJvrcWalkEnv(spec, seed=3, env_id=i) for i in range(n)]


@pytest.mark.parametrize("name", ["stilts", "sphere_inside_box", "parallel_capsules"])
def test_degenerate_narrow_phase_branches_on_the_emulator(tmp_path, name):
    from tests import emu
    spec, q, check = _case(tmp_path, name)
    env = emu.make_emulated(spec, len(q), seed=3)

    def step(a):
        _, rew, done, _ = env.step(a)
        return rew, done
    _run(spec, q, check, env, _oracles(spec, len(q)), step, lambda: env.rew_terms.numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["stilts", "sphere_inside_box", "parallel_capsules"])
def test_degenerate_narrow_phase_branches_on_the_gpu(tmp_path, name):
    import torch
    spec, q, check = _case(tmp_path, name)
    env = spec.make_batched(len(q), seed=3, device=0)

    def step(a):
        _, rew, done, _ = env.step(torch.from_numpy(a).cuda())
        return rew.cpu().numpy(), done.cpu().numpy()
    _run(spec, q, check, env, _oracles(spec, len(q)), step, lambda: env.rew_terms.cpu().numpy())
