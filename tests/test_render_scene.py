"""lhw_render_scene (csrc/lhw_render.hip) on the SIMT emulator against the float64 ray caster of tests/render_scene_oracle.py -- the cone,
translucent layers, dynamic geoms, three passes of 64 geoms -- and the host side of the markers: markers.Markers / walk_markers /
step_terrain and the eval parser's --render-markers."""
import math

import numpy as np
import pytest
import torch

from learninghumanoidwalking_amd import _lib, markers
from learninghumanoidwalking_amd.markers import Markers
from learninghumanoidwalking_amd.render import Renderer
from tests import render_checks as C
from tests import render_scene_checks as S
from tests import render_scene_oracle as O


def make(gtype, size, rgba, W, H, **settings):
    from tests import render_emu
    return Renderer.from_geoms(gtype, size, rgba, W, H, device="cpu", library=render_emu.lib(), **settings)


def guarded(W, H, F=1, device="cpu"):
    """the five outputs as views of 0xA5-filled buffers with 64 guard bytes behind each: (raw buffers, bytes per pixel, views)"""
    n = F * W * H
    per = (3, 4, 4, 4, 4)
    raw = [torch.full((n * k + 64,), 0xA5, dtype=torch.uint8, device=device) for k in per]
    out = (raw[0][:n * 3].view(F, H, W, 3), raw[1][:n * 4].view(torch.int32).view(F, H, W), raw[2][:n * 4].view(torch.float32).view(F, H, W),
           raw[3][:n * 4].view(torch.int32).view(F, H, W), raw[4][:n * 4].view(torch.int32).view(F, H, W))
    return raw, per, out


def test_scenes_are_stable_enough_and_the_depth_tolerance_is_the_measured_one():
    """oracle alone: every scene keeps its unstable share below the cap, and DEPTH_RTOL is 8 x the float32 error of the oracle's formulas"""
    res = S.measure_depth_error()
    for name, (err, unstable) in res.items():
        print(f"{name}: float32 depth error {err:.3e}, unstable {unstable:.4f}")
        assert unstable <= O.MAX_UNSTABLE, name
    worst = max(e for e, _ in res.values())
    # (the float32 run's last bits follow the host's BLAS, so the recorded figure is held to the re-measured one within a factor of two)
    assert 0.5 * worst <= O.MEASURED_F32_DEPTH_ERROR <= 2 * worst and O.DEPTH_RTOL == 8 * O.MEASURED_F32_DEPTH_ERROR, worst
    assert O.MAX_UNSTABLE == 0.03 and O.MAX_LAYERS == _lib.RENDER_MAX_LAYERS and O.CONE == _lib.RENDER_CONE and O.MAX_GEOMS == _lib.RENDER_SCENE_MAX_GEOMS


@pytest.mark.parametrize("name", ["single_cone_axis", "single_cone_rot", "arrow_end", "arrow_side"])
def test_cone_and_arrow(name):
    S.check_against_oracle(make, name, min_cover=0.03)
    parts = np.unique(S.oracle(name)["hit"][S.oracle(name)["hit"] >= 0] % 8).tolist()
    if name == "arrow_side":
        assert len(np.unique(S.oracle(name)["hit"] // 8)) == 3      # background, shaft, head
    if name == "arrow_end":
        assert parts == [0]                                        # seen from the tip: the lateral surface alone
    if name == "single_cone_rot":
        assert parts == [0, 1]                                     # lateral surface and base


def test_layers_over_the_seven_geom_scene():
    ref = S.oracle("layers_seven")
    rgb, hit, depth, layers, layer_hit = (x[0] for x in S.check_against_oracle(make, "layers_seven"))
    assert ((layers == 2) & ref["stable"]).any() and ref["shadow"].mean() > 0.02 and len(np.unique(ref["parity"])) == 2
    # the translucent box (id 10) behind the ellipsoid (id 4) shows beside it and contributes nothing where the ellipsoid covers it
    ids = ref["layer_list"] // 8
    assert (ids == 10).any() and not (ids == 10)[:, ref["hit"] // 8 == 4].any()
    assert (layers[(hit // 8 == 4) & ref["stable"]] == 0).any()
    # the order of two layers matters: the same two spheres with colour and alpha exchanged give other colours where both cover a pixel
    other = S.oracle("layers_seven_swapped")
    both = ref["stable"] & other["stable"] & (ref["layers"] == 2) & (other["layers"] == 2)
    assert both.sum() >= 5 and (np.abs(ref["rgb"][both].astype(int) - other["rgb"][both].astype(int)).max(axis=-1) > 4).all()
    S.check_against_oracle(make, "layers_seven_swapped")


def test_ten_layers_keep_the_nearest_eight():
    ref = S.oracle("layers_ten")
    rgb, hit, depth, layers, layer_hit = (x[0] for x in S.check_against_oracle(make, "layers_ten"))
    ten = ref["stable"] & (ref["in_front"] == 10)
    assert ten.sum() > 20 and (layers[ten] == 8).all() and (ref["stable"] & (ref["in_front"] == 8)).any()
    ids = ref["layer_list"][:, ten] // 8      # the slabs are ids 7 (farthest) .. 16 (nearest)
    assert (ids == np.arange(16, 8, -1)[:, None]).all() and (layer_hit[ten] // 8 == 16).all()


def test_three_passes_of_geoms_and_a_shadow_across_them():
    ref = S.oracle("grid130")
    rgb, hit, depth, layers, layer_hit = (x[0] for x in S.check_against_oracle(make, "grid130"))
    assert sorted(np.unique(hit[hit >= 0] // 8).tolist()) == list(range(130))
    on5 = ref["stable"] & (ref["hit"] // 8 == S.GRID_SHADOWED)
    assert (ref["shadow"] & on5).any() and (layers == 0).all() and (layer_hit == -1).all()
    c = S.case("grid130")      # ... and it is geom 129's shadow: without it geom 5 is lit
    sc = O.frame_scene(c["static"], c["dynamic"], 0)
    sc["rgba"][S.GRID_OCCLUDER, 3] = 0.0
    assert not (O.render(sc, c["cams"][0][0], c["cams"][0][1], c["W"], c["H"], stable=False)["shadow"] & on5).any()


def test_dynamic_geoms_of_three_frames():
    full = S.check_against_oracle(make, "dynamic_three")
    assert [int(S.oracle("dynamic_three", f)["layers"].max()) for f in range(3)] == [0, 0, 1]
    assert [bool((S.oracle("dynamic_three", f)["hit"] // 8 == 4).any()) for f in range(3)] == [True, False, True]      # the marker is absent in frame 1
    for f in range(3):
        one = S.draw(make, "dynamic_three", frames=slice(f, f + 1))
        for a, b in zip(full, one):
            assert np.array_equal(a[f], b[0], equal_nan=True), f


def test_clipped_tiles_write_inside_the_image_only():
    c = S.case("odd_layers")
    raw, per, out = guarded(c["W"], c["H"])
    images = S.draw(make, "odd_layers", out=out)
    for r, k in zip(raw, per):
        assert (r[c["W"] * c["H"] * k:] == 0xA5).all()
    S.check_against_oracle(make, "odd_layers", images=images, min_cover=0.05)
    ref = S.oracle("odd_layers")
    assert (ref["layers"][:, 32:] > 0).any() and (ref["layers"][16:, :] > 0).any()      # the translucent sphere lies over the clipped tiles


def test_culling_changes_no_bit():
    for name in ("layers_seven", "grid130"):
        on, off = S.draw(make, name), S.draw(make, name, cull=False)
        for a, b in zip(on, off):
            assert np.array_equal(a, b), name


def _refused(static, dynamic, code):
    r = make(static["type"], static["size"], static["rgba"], 16, 8)
    raw, per, out = guarded(16, 8, F=dynamic["type"].shape[0])
    F = dynamic["type"].shape[0]
    cp, cr = C.camera()
    with pytest.raises(_lib.LhwError) as e:
        r.render_scene(static["pos"], static["mat"], np.repeat(cp[None], F, 0), np.repeat(cr[None], F, 0), dynamic=dynamic, out=out)
    assert e.value.code == code
    for b in raw:
        assert (b == 0xA5).all()


def test_refusals_write_nothing():
    ball = lambda k: (O.SPHERE, (0.1,), C.RED, (0.01 * k, 0, 0), np.eye(3))
    _refused(S._static([ball(k) for k in range(200)]), S._dynamic([[ball(k) for k in range(57)]]), -4)      # 257 geoms: LHW_ERR_UNSUPPORTED
    frames = [[ball(0), ball(1)] for _ in range(3)]
    frames[2][1] = (7, (0.1,), C.RED, (0, 0, 0), np.eye(3))                                                  # type 7 (a mesh) in frame 2
    _refused(S._static([ball(0)], F=3), S._dynamic(frames), -1)
    _refused(S._static([]), S._dynamic([[(O.CONE, (0.2, 0.0), C.RED, (0, 0, 0), np.eye(3))]]), -1)           # a drawn cone with hl = 0
    # ... which is fine while it is absent (alpha 0), and 256 geoms are taken
    r = make(np.zeros(0), np.zeros((0, 3)), np.zeros((0, 4)), 16, 8)
    cp, cr = C.camera()
    r.render_scene(np.zeros((1, 0, 3)), np.zeros((1, 0, 9)), cp[None], cr[None], dynamic=S._dynamic([[(O.CONE, (0.2, 0.0), S.alpha(C.RED, 0.0), (0, 0, 0), np.eye(3))]]))
    st = S._static([ball(k) for k in range(200)])
    make(st["type"], st["size"], st["rgba"], 16, 8).render_scene(st["pos"], st["mat"], cp[None], cr[None], dynamic=S._dynamic([[ball(k) for k in range(56)]]))


def test_opaque_static_scene_equals_lhw_render_frames():
    """the 9 geoms of jvrc_walk, no dynamic geom, alpha 1: the scene entry returns lhw_render_frames' bytes"""
    from learninghumanoidwalking_amd.envs import ENVIRONMENTS
    from tests import render_emu
    spec = ENVIRONMENTS["jvrc_walk"]()
    r = Renderer(spec.model(), 64, 48, device="cpu", library=render_emu.lib())
    assert r.n_geoms == 9
    q = np.stack([spec.nominal_pose, spec.nominal_pose])
    q[1, 0] += 3.3
    old = r.render(q, aux=True)
    new = r.render(q, aux=True, markers=Markers())
    assert len(old) == 3 and len(new) == 5
    for a, b in zip(old, new[:3]):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert (new[3] == 0).all() and (new[4] == -1).all() and len(torch.unique(old[1])) > 5
    assert torch.equal(r.render(q), r.render_scene(*_poses(r, q)))      # dynamic=None: the old entry


def _poses(r, q):
    from learninghumanoidwalking_amd.kinematics import body_poses, geom_poses
    from learninghumanoidwalking_amd.render import TrackingCamera
    pos, mat = geom_poses(r.model, q)
    return (pos, mat) + TrackingCamera().poses(body_poses(r.model, q)[0])


def test_a_library_without_the_scene_entry_is_reported():
    from tests import render_emu

    class Old:      # a build of the ABI from before lhw_render_scene
        def __getattr__(self, name):
            if name == "lhw_render_scene":
                raise AttributeError(name)
            return getattr(render_emu.lib(), name)

    r = Renderer.from_geoms([O.SPHERE], [(0.5, 0, 0)], [C.RED], 16, 8, device="cpu", library=Old())
    cp, cr = C.camera()
    r.render_scene(np.zeros((1, 1, 3)), np.eye(3).reshape(1, 1, 9), cp[None], cr[None])
    with pytest.raises(_lib.LhwError) as e:
        r.render_scene(np.zeros((1, 1, 3)), np.eye(3).reshape(1, 1, 9), cp[None], cr[None], dynamic=Markers())
    assert e.value.code == -4 and "lhw_render_scene" in str(e.value)


# ---- host only

def test_arrow_geometry():
    for L, head, shaft in ((0.5, 0.2, 0.3), (0.05, 0.05, None), (-0.3, 0.2, 0.1), (0.0, None, None)):
        a = Markers().arrow(0, (1.0, 2.0, 3.0), (0.0, 0.0, 1.0), 0.05, L, (0, 0, 1, 0.5)).arrays(1)
        live = a["rgba"][0, :, 3] != 0
        types = a["type"][0][live].tolist()
        assert types == ([] if head is None else ([markers.CYLINDER] if shaft else []) + [markers.CONE]), L
        if head is None:
            continue
        sgn = 1.0 if L > 0 else -1.0
        cone = types.index(markers.CONE)
        np.testing.assert_allclose(a["size"][0, cone, :2], (0.1, head / 2), atol=1e-15)      # base radius 2 r, half height h / 2
        z = a["mat"][0, cone].reshape(3, 3)[:, 2]
        np.testing.assert_allclose(z, (0, 0, sgn), atol=1e-15)
        np.testing.assert_allclose(a["pos"][0, cone] + z * head / 2, (1.0, 2.0, 3.0 + L), atol=1e-15)      # the apex is the arrow's tip
        if shaft:
            np.testing.assert_allclose(a["size"][0, 0, :2], (0.05, shaft / 2), atol=1e-15)
            np.testing.assert_allclose(a["pos"][0, 0], (1.0, 2.0, 3.0 + sgn * shaft / 2), atol=1e-15)
        R = a["mat"][0, cone].reshape(3, 3)
        np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-15)
        assert np.linalg.det(R) > 0
    a = Markers().add(0, markers.SPHERE, (0.1,), C.RED, (0, 0, 0)).add(2, markers.BOX, (0.1, 0.2, 0.3), C.BLUE, (1, 0, 0)).add(2, markers.SPHERE, (0.2,), C.RED, (0, 1, 0)).arrays(3)
    assert a["type"].shape == (3, 2) and a["rgba"][:, :, 3].tolist() == [[1, 0], [0, 0], [1, 1]] and (a["size"][a["rgba"][:, :, 3] == 0] > 0).all()


def test_walk_markers_per_mode():
    F = _lib.TASK_INPUT_FIELDS
    rows = np.zeros((3, _lib.TASK_INPUT_DIM))
    yaw = 0.7
    for r, mode in zip(rows, (markers.MODE_STANDING, markers.MODE_INPLACE, markers.MODE_FORWARD)):
        r[F["mode"][0]] = mode
        r[F["head_xpos"][0]:F["head_xpos"][0] + 3] = (1.0, 2.0, 1.5)
        r[F["qpos"][0] + 3:F["qpos"][0] + 7] = (math.cos(yaw / 2), 0, 0, math.sin(yaw / 2))
        r[F["mode_ref"][0]:F["mode_ref"][0] + 3] = (0.3, 0.4, 0.0)
        r[F["qvel"][0]:F["qvel"][0] + 6] = (0.0, 0.25, 0.0, 0, 0, -0.2)
    a = markers.walk_markers(rows).arrays(3)
    live = a["rgba"][:, :, 3] != 0
    assert live.sum(axis=1).tolist() == [0, 4, 4]      # standing: none; otherwise two arrows of shaft + head
    assert {markers.MODE_STANDING, markers.MODE_INPLACE, markers.MODE_FORWARD} == {0, 1, 2}      # csrc/lhw_humanoid_dev.h: MODE_STANDING 0, MODE_INPLACE 1, MODE_FORWARD 2
    tip = lambda f, m: a["pos"][f, m] + a["mat"][f, m].reshape(3, 3)[:, 2] * a["size"][f, m, 1]
    at = np.array([1.0, 2.0, 1.8])
    # INPLACE: the command 2 * 0.3 up, the measurement 2 * 0.2 DOWN (qvel[5] < 0)
    np.testing.assert_allclose(tip(1, 1), at + [0, 0, 0.6], atol=1e-12)
    np.testing.assert_allclose(tip(1, 3), at - [0, 0, 0.4], atol=1e-12)
    # FORWARD: the command 2 * 0.4 along the heading, the measurement 2 * 0.25 along +y
    np.testing.assert_allclose(tip(2, 1), at + 0.8 * np.array([math.cos(yaw), math.sin(yaw), 0]), atol=1e-12)
    np.testing.assert_allclose(tip(2, 3), at + [0, 0.5, 0], atol=1e-12)
    assert a["rgba"][2, 0].tolist() == [0, 0, 1, 0.5] and a["rgba"][2, 2].tolist() == [0, 1, 0, 0.5] and (a["size"][2, [0, 2], 0] == 0.05).all()


def test_step_terrain_box_poses():
    rng = np.random.default_rng(3)
    seq = np.zeros((2, 20, 6))
    seq[:, :, :4] = rng.normal(size=(2, 20, 4))
    nseq, floor_z, bh = np.array([20, 7]), np.array([0.0, -2.0]), 0.05 + 0.01 * np.arange(20)
    a = markers.step_terrain(seq, nseq, floor_z, bh).arrays(2)
    assert a["type"].shape == (2, 21) and (a["type"][:, :20] == markers.BOX).all() and (a["type"][:, 20] == markers.PLANE).all()
    for f in range(2):
        # tasks/stepping_task.py:320-334: sequence = [(0, 0, -1, 0)] * 20 with the episode's steps in front; box.pos = step[:3] - (0, 0, box_h),
        # box.quat = euler2quat(0, 0, step[3]), size (0.15, 1, box_h), rgba (0.8, 0.8, 0.8, 1)
        steps = [np.array([0, 0, -1.0, 0])] * 20
        steps[:nseq[f]] = list(seq[f, :nseq[f], :4])
        for i, step in enumerate(steps):
            np.testing.assert_allclose(a["pos"][f, i], step[:3] - [0, 0, bh[i]], atol=1e-15)
            c, s = math.cos(step[3]), math.sin(step[3])
            np.testing.assert_allclose(a["mat"][f, i].reshape(3, 3), [[c, -s, 0], [s, c, 0], [0, 0, 1]], atol=1e-15)
            assert a["size"][f, i].tolist() == [0.15, 1.0, bh[i]] and a["rgba"][f, i].tolist() == [0.8, 0.8, 0.8, 1.0]
        assert a["pos"][f, 20].tolist() == [0, 0, floor_z[f]] and a["rgba"][f, 20, 3] == 1.0


def test_eval_command_line_defaults_to_no_markers():
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("run_experiment_cli", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "run_experiment.py"))
    rx = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rx)
    assert rx.build_eval_parser().parse_args(["--path", "x"]).render_markers is False
    assert rx.build_eval_parser().parse_args(["--path", "x", "--render-markers"]).render_markers is True
