"""lhw_render_frames (csrc/lhw_render.hip) on the SIMT emulator against the float64 ray caster of tests/render_oracle.py, and the host
side of the frames: kinematics.geom_poses, render.TrackingCamera / write_png, the geom colours mjcf.py reads."""
import struct
import zlib

import numpy as np
import pytest
import torch

from learninghumanoidwalking_amd import _lib, mjcf
from learninghumanoidwalking_amd.model import GEOM_PALETTE
from learninghumanoidwalking_amd.render import Renderer, TrackingCamera, write_png
from tests import render_checks as C
from tests import render_oracle as O


def make(gtype, size, rgba, W, H, **settings):
    from tests import render_emu
    return Renderer.from_geoms(gtype, size, rgba, W, H, device="cpu", library=render_emu.lib(), **settings)


def test_scenes_are_stable_enough_and_the_depth_tolerance_is_the_measured_one():
    """oracle alone: every scene keeps its unstable share below the cap, and DEPTH_RTOL is 8 x the float32 error of the oracle's formulas"""
    res = C.measure_depth_error()
    for name, (err, unstable) in res.items():
        print(f"{name}: float32 depth error {err:.3e}, unstable {unstable:.4f}")
        assert unstable <= O.MAX_UNSTABLE, name
    worst = max(e for e, _ in res.values())
    # (the float32 run's last bits follow the host's BLAS, so the recorded figure is held to the re-measured one within a factor of two)
    assert 0.5 * worst <= O.MEASURED_F32_DEPTH_ERROR <= 2 * worst and O.DEPTH_RTOL == 8 * O.MEASURED_F32_DEPTH_ERROR, worst


@pytest.mark.parametrize("how", ["axis", "rot"])
@pytest.mark.parametrize("prim", list(C.PRIMITIVES))
def test_single_primitive(prim, how):
    C.check_against_oracle(make, f"single_{prim}_{how}", min_cover=0.05)


def test_seven_geom_scene_with_shadows_and_checkerboard():
    ref = C.oracle("seven")
    assert ref["shadow"].mean() > 0.02 and len(np.unique(ref["parity"])) == 2 and len(np.unique(ref["hit"] // 8)) == 7      # the scene exercises them
    C.check_against_oracle(make, "seven")


def test_culling_changes_no_bit():
    for name in ("seven", "seven_plus"):
        on, off = C.draw(make, name), C.draw(make, name, cull=False)
        for a, b in zip(on, off):
            assert np.array_equal(a, b), name
        C.check_against_oracle(make, name, images=on)
    hit = C.oracle("seven_plus")["hit"] // 8
    assert (hit == 7).sum() > 20 and (hit == 8).sum() > 100      # the thin capsule and the large ellipsoid are in the picture


@pytest.mark.parametrize("name", ["odd_box", "odd_capsule"])
def test_clipped_tiles_write_inside_the_image_only(name):
    W, H = C.case(name)[2:4]
    n = W * H
    raw = [torch.full((n * k + 64,), 0xA5, dtype=torch.uint8) for k in (3, 4, 4)]
    out = (raw[0][:n * 3].view(1, H, W, 3), raw[1][:n * 4].view(torch.int32).view(1, H, W), raw[2][:n * 4].view(torch.float32).view(1, H, W))
    images = C.draw(make, name, out=out)
    for r, k in zip(raw, (3, 4, 4)):
        assert (r[n * k:] == 0xA5).all()
    C.check_against_oracle(make, name, images=images, min_cover=0.05)


def test_frames_of_one_call_equal_single_frame_calls():
    sc = C.case("seven")[0]
    cams = [C.camera(lookat=(0.1, 0.0, 0.45), distance=4.0, azimuth=70.0, elevation=-25.0), C.camera(lookat=(0, 0, 0.3), distance=3.0, azimuth=120.0, elevation=-40.0),
            C.camera(lookat=(50.3, -20.0, 0.5), distance=5.0, azimuth=10.0, elevation=-15.0)]
    pos = np.stack([sc["pos"], sc["pos"] + [0.2, -0.1, 0.05], sc["pos"] + [50.0, -20.0, 0.0]])
    pos[:, :2] = sc["pos"][:2]                                      # (the floor and the wall stay)
    mat = np.stack([sc["mat"], sc["mat"], np.einsum("ij,gjk->gik", C.rot((0, 0, 1.0), 0.3), sc["mat"])]).reshape(3, -1, 9)
    mat[2, :2] = sc["mat"][:2].reshape(2, 9)
    r = make(sc["type"], sc["size"], sc["rgba"], 40, 24)
    cp, cr = np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams])
    full = r.render_geoms(pos, mat, cp, cr, aux=True)
    assert len(torch.unique(full[1][2] // 8)) >= 5                  # the frame 50 m from the origin shows the scene too
    for f in range(3):
        one = r.render_geoms(pos[f:f + 1], mat[f:f + 1], cp[f:f + 1], cr[f:f + 1], aux=True)
        for a, b in zip(full, one):
            assert torch.equal(a[f], b[0]), f


def test_sixty_four_geoms_fill_the_mask():
    rgb, hit, depth = C.check_against_oracle(make, "grid64")
    assert sorted(np.unique(hit[hit >= 0] // 8).tolist()) == list(range(64))


def test_sixty_five_geoms_are_refused_with_nothing_written():
    sc = C._grid64(65)
    r = make(sc["type"], sc["size"], sc["rgba"], 16, 8)
    out = (torch.full((1, 8, 16, 3), 0xA5, dtype=torch.uint8), torch.full((1, 8, 16), -7, dtype=torch.int32), torch.full((1, 8, 16), -7.0))
    cp, cr = C.camera(distance=5.0, elevation=0.0)
    with pytest.raises(_lib.LhwError) as e:
        r.render_geoms(sc["pos"][None], sc["mat"].reshape(1, -1, 9), cp[None], cr[None], out=out)
    assert e.value.code == -4      # LHW_ERR_UNSUPPORTED
    assert (out[0] == 0xA5).all() and (out[1] == -7).all() and (out[2] == -7.0).all()


def test_bad_type_or_size_is_refused_with_nothing_written():
    cp, cr = C.camera()
    for gtype, size in ((1, (0.5, 0, 0)), (O.SPHERE, (0.0, 0, 0)), (O.BOX, (0.5, -0.1, 0.2))):
        r = make([gtype], [size], [C.RED], 16, 8)
        out = (torch.full((1, 8, 16, 3), 0xA5, dtype=torch.uint8), None, None)
        with pytest.raises(_lib.LhwError) as e:
            r.render_geoms(np.zeros((1, 1, 3)), np.eye(3).reshape(1, 1, 9), cp[None], cr[None], out=out)
        assert e.value.code == -1 and (out[0] == 0xA5).all()


def test_behind_the_camera_below_the_plane_and_alpha_zero():
    cp, cr = C.camera(lookat=(0, 0, 0), distance=3.0, azimuth=90.0, elevation=-20.0)
    fwd = cr[6:]
    behind = cp - 2.0 * fwd
    sc = C.scene_of([(O.SPHERE, (0.5,), C.RED, behind, np.eye(3)), (O.SPHERE, (0.4,), (0.2, 0.9, 0.2, 0.0), (0, 0, 0), np.eye(3)), (O.BOX, (0.2, 0.2, 0.2), C.BLUE, (0.9, 0, 0), np.eye(3))])
    r = make(sc["type"], sc["size"], sc["rgba"], 32, 24)
    rgb, hit, depth = (x[0].numpy() for x in r.render_geoms(sc["pos"][None], sc["mat"].reshape(1, -1, 9), cp[None], cr[None], aux=True))
    assert set(np.unique(hit // 8).tolist()) == {-1, 2}            # neither the sphere behind the camera nor the transparent one
    ref = O.render(sc, cp, cr, 32, 24)
    assert np.array_equal(hit[ref["stable"]], ref["hit"][ref["stable"]])
    # a plane seen from below shows its underside lit from below: the normal is flipped towards the viewer
    cp, cr = C.camera(lookat=(0, 0, 0), distance=3.0, azimuth=90.0, elevation=50.0)      # the camera is under z = 0 and looks up
    sc = C.scene_of([(O.PLANE, (0, 0, 0), C.GREY, (0, 0, 0), np.eye(3))])
    imgs = {}
    for name, light in (("from_below", (0.2, 0.1, -1.0)), ("from_above", (0.2, 0.1, 1.0))):
        r = make(sc["type"], sc["size"], sc["rgba"], 16, 8, light_dir=light, shadows=False, checker_size=0.0)
        rgb, hit, _ = (x[0].numpy() for x in r.render_geoms(sc["pos"][None], sc["mat"].reshape(1, -1, 9), cp[None], cr[None], aux=True))
        ref = O.render(sc, cp, cr, 16, 8, dict(light_dir=light, shadows=False, checker_size=0.0))
        assert (hit == 0).all() and np.abs(rgb.astype(int) - ref["rgb"].astype(int)).max() <= 1
        imgs[name] = rgb
    assert imgs["from_below"].min() > imgs["from_above"].max()     # lit underside against ambient only


def test_tracking_camera_is_the_documented_one():
    cam = TrackingCamera()
    assert (cam.distance, cam.azimuth, cam.elevation, cam.lookat_body) == (4.0, 90.0, -20.0, 1)
    xpos = np.array([[[0, 0, 0], [1.0, 2.0, 0.9]], [[0, 0, 0], [50.0, -3.0, 0.8]]])
    pos, rows = cam.poses(xpos)
    for f in range(2):
        p, r = C.camera(lookat=xpos[f, 1], distance=4.0, azimuth=90.0, elevation=-20.0)
        np.testing.assert_allclose(pos[f], p, atol=1e-15)
        np.testing.assert_allclose(rows[f], r, atol=1e-15)
    R = rows[0].reshape(3, 3)
    np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-15)


@pytest.mark.parametrize("env", ["jvrc_walk", "h1"])
def test_geom_poses_agree_with_the_emulated_stepper(env):
    from learninghumanoidwalking_amd.envs import ENVIRONMENTS
    from learninghumanoidwalking_amd.kinematics import _quat_mul, body_poses, geom_poses
    from tests import emu
    spec = ENVIRONMENTS[env]()
    N = 2
    e = emu.make_emulated(spec, N, seed=3)
    e.enable_task_inputs(True)
    e.reset()
    m = e.model
    ids = dict(zip(("root", "head", "rfoot", "lfoot"), spec.body_ids()))
    rng = np.random.default_rng(5)
    dt = m.timestep
    for _ in range(3):
        e.step((0.3 * rng.normal(size=(N, e.act_dim))).astype(np.float32))
        rec = e.get_task_inputs()
        # The record's body frames are those of the control step's LAST FORWARD PASS, its qpos / qvel the state after the integration that
        # followed it (include/lhw.h, LhwTaskInput: MuJoCo's staleness).  The semi-implicit Euler step is qpos' = qpos (+) dt qvel', so the
        # qpos of that forward pass is the record's, taken back by the record's own velocity (the root's angular velocity is body-fixed).
        q, v = rec["qpos"].copy(), rec["qvel"]
        q[:, :3] -= dt * v[:, :3]
        q[:, 7:] -= dt * v[:, 6:]
        w = -dt * v[:, 3:6]
        ang = np.linalg.norm(w, axis=1, keepdims=True)
        dq = np.concatenate([np.cos(0.5 * ang), np.sin(0.5 * ang) * w / np.maximum(ang, 1e-300)], axis=1)
        q[:, 3:7] = _quat_mul(rec["qpos"][:, 3:7], dq)
        xpos, _, xmat = body_poses(m, q)
        for key, b in ids.items():
            err = np.abs(xpos[:, b] - rec[key + "_xpos"]).max()
            print(env, key, "|FK(qpos of the last forward pass) - record|", err, "  |FK(record qpos) - record|", np.abs(body_poses(m, rec["qpos"])[0][:, b] - rec[key + "_xpos"]).max())
            assert err <= 1e-12, (key, err)
        err = np.abs(xmat[:, ids["root"]].reshape(N, 9) - rec["root_xmat"]).max()
        print(env, "root_xmat", err)
        assert err <= 1e-12
        pos, mat = geom_poses(m, rec["qpos"])
        assert pos.shape == (N, m.ngeom, 3) and mat.shape == (N, m.ngeom, 9)


def _decode_png(path):
    """an 8-bit RGB / grey PNG without interlace, every filter type"""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, head = 8, b"", None
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF
        if tag == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    assert tag == b"IEND"
    w, h, depth, colour, comp, filt, lace = head
    assert (depth, comp, filt, lace) == (8, 0, 0, 0) and colour in (0, 2)
    ch = 3 if colour == 2 else 1
    raw = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + w * ch)
    assert (raw[:, 0] == 0).all()      # write_png uses filter 0 on every row
    img = raw[:, 1:].reshape(h, w, ch)
    return img if ch == 3 else img[:, :, 0]


@pytest.mark.parametrize("w", [1, 37, 64])
def test_write_png_round_trip(tmp_path, w):
    rng = np.random.default_rng(w)
    a = rng.integers(0, 256, size=(5 if w == 1 else 21, w, 3), dtype=np.uint8)
    write_png(tmp_path / "a.png", a)
    assert np.array_equal(_decode_png(tmp_path / "a.png"), a)
    write_png(tmp_path / "t.png", torch.from_numpy(a))
    assert (tmp_path / "t.png").read_bytes() == (tmp_path / "a.png").read_bytes()
    write_png(tmp_path / "g.png", a[:, :, 0])
    assert np.array_equal(_decode_png(tmp_path / "g.png"), a[:, :, 0])
    with pytest.raises(ValueError):
        write_png(tmp_path / "bad.png", a.astype(np.float32))


_RGBA_XML = """<mujoco><compiler angle="radian"/>
<default><default class="blue"><geom rgba="0.1 0.2 0.9 1"/></default></default>
<worldbody>
 <geom name="floor" type="plane" size="0 0 1"/>
 <body name="a" pos="0 0 1"><freejoint/>
  <geom name="plain" type="sphere" size="0.1"/>
  <geom name="own" type="sphere" size="0.1" pos="0.3 0 0" rgba="0.9 0.8 0.1 0.5"/>
  <geom name="classed" class="blue" type="sphere" size="0.1" pos="0.6 0 0"/>
  <body name="b" pos="0 0 0.3"><joint type="hinge" axis="0 1 0"/><geom name="child" type="capsule" size="0.05 0.1"/></body>
 </body>
</worldbody></mujoco>"""


def test_geom_colours_from_mjcf():
    m = mjcf.compile_string(_RGBA_XML)
    c = {n: tuple(m.geom_rgba[m.geom_id(n)]) for n in m.geom_names}
    assert c["floor"] == (0.5, 0.5, 0.5, 1.0)
    assert c["own"] == (0.9, 0.8, 0.1, 0.5) and c["classed"] == (0.1, 0.2, 0.9, 1.0)
    assert c["plain"] == GEOM_PALETTE[m.body_id("a") % 8] + (1.0,) and c["child"] == GEOM_PALETTE[m.body_id("b") % 8] + (1.0,)
    assert c["plain"] != c["child"] and len(set(GEOM_PALETTE)) == 8
    iblob, dblob = m.pack()                                      # the packed layout does not carry the colours
    m.geom_rgba = None
    assert all(np.array_equal(x, y) for x, y in zip(m.pack(), (iblob, dblob)))
    # the stand-in robots: left and right legs differ
    from learninghumanoidwalking_amd.envs import ENVIRONMENTS
    spec = ENVIRONMENTS["jvrc_walk"]()
    mm = spec.model()
    r, l = (mm.geom_rgba[np.asarray(mm.geom_bodyid) == b][0] for b in spec.body_ids()[2:])
    assert not np.array_equal(r, l) and mm.geom_rgba.shape == (mm.ngeom, 4)


def test_renderer_on_a_model_through_the_emulator():
    """Renderer(model).render(qpos): kinematics, camera and kernel together show the robot standing on the floor"""
    from learninghumanoidwalking_amd.envs import ENVIRONMENTS
    from tests import render_emu
    spec = ENVIRONMENTS["jvrc_walk"]()
    m = spec.model()
    r = Renderer(m, 64, 48, device="cpu", library=render_emu.lib())
    q = np.stack([spec.nominal_pose, spec.nominal_pose])
    q[1, 0] += 50.0                                              # 50 m down the track: the same picture up to the checkerboard's phase
    rgb, hit, depth = r.render(q, aux=True)
    assert rgb.shape == (2, 48, 64, 3) and rgb.dtype == torch.uint8
    planes = torch.tensor([g for g in range(m.ngeom) if m.geom_type[g] == O.PLANE])
    robot = (hit >= 0) & ~torch.isin(hit // 8, planes)
    assert 0.003 <= robot[0].float().mean() <= 0.5 and len(torch.unique(hit[0][robot[0]] // 8)) >= 6      # (the stand-in is a pair of legs, 4 m away)
    assert (hit[0] >= 0).float().mean() >= 0.02 and (hit[0] < 0).any()                                       # floor below, background above the horizon
    assert torch.equal(hit[0], hit[1]) and torch.allclose(depth[0], depth[1], rtol=1e-5)
    assert r.frames_per_chunk == (64 * 2 ** 20 - 1) // (64 * 48 * 3)


def test_eval_command_line_defaults_to_no_frames():
    import argparse
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("run_experiment_cli", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "run_experiment.py"))
    rx = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rx)
    ea = rx.build_eval_parser().parse_args(["--path", "x"])
    assert (ea.render_envs, ea.render_size, ea.render_every) == (0, (640, 480), 1)
    ea = rx.build_eval_parser().parse_args(["--path", "x", "--render-envs", "2", "--render-size", "64x48", "--render-every", "5"])
    assert (ea.render_envs, ea.render_size, ea.render_every) == (2, (64, 48), 5)
    for bad in ("64", "0x48", "axb"):
        with pytest.raises(argparse.ArgumentTypeError):
            rx._size(bad)
    with pytest.raises(SystemExit, match="--render-envs needs --out-dir"):
        rx.run_eval(["--path", "x", "--render-envs", "1"])
