"""lhw_render_frames on the GPU against the float64 ray caster of tests/render_oracle.py (the cases of tests/test_render.py that depend
on the device: lane mapping, ballot, LDS output path, clipped tiles, a full geom mask), and `run_experiment.py eval --render-envs`."""
import json

import numpy as np
import pytest
import torch

from learninghumanoidwalking_amd.render import Renderer
from tests import render_checks as C
from tests.test_render import _decode_png

pytestmark = pytest.mark.gpu


def make(gtype, size, rgba, W, H, **settings):
    return Renderer.from_geoms(gtype, size, rgba, W, H, device=0, **settings)


@pytest.mark.parametrize("how", ["axis", "rot"])
@pytest.mark.parametrize("prim", ["box", "capsule"])
def test_single_primitive(prim, how):
    C.check_against_oracle(make, f"single_{prim}_{how}", min_cover=0.05)


def test_seven_geom_scene_and_culling_changes_no_bit():
    for name in ("seven", "seven_plus"):
        on, off = C.draw(make, name), C.draw(make, name, cull=False)
        for a, b in zip(on, off):
            assert np.array_equal(a, b), name
        C.check_against_oracle(make, name, images=on)


@pytest.mark.parametrize("name", ["odd_box", "odd_capsule"])
def test_clipped_tiles_write_inside_the_image_only(name):
    W, H = C.case(name)[2:4]
    n = W * H
    raw = [torch.full((n * k + 64,), 0xA5, dtype=torch.uint8, device="cuda") for k in (3, 4, 4)]
    out = (raw[0][:n * 3].view(1, H, W, 3), raw[1][:n * 4].view(torch.int32).view(1, H, W), raw[2][:n * 4].view(torch.float32).view(1, H, W))
    images = C.draw(make, name, out=out)
    for r, k in zip(raw, (3, 4, 4)):
        assert (r[n * k:] == 0xA5).all()
    C.check_against_oracle(make, name, images=images, min_cover=0.05)


def test_sixty_four_geoms_fill_the_mask():
    rgb, hit, depth = C.check_against_oracle(make, "grid64")
    assert sorted(np.unique(hit[hit >= 0] // 8).tolist()) == list(range(64))


def test_eval_writes_frames(tmp_path):
    from learninghumanoidwalking_amd.envs import ENVIRONMENTS
    from tests.test_eval_cli_gpu import _run, _train
    logs, run = _train(tmp_path, "jvrc_walk")
    base = ["eval", "--logdir", str(logs), "--ep-len", "0.2", "--num-envs", "4", "--seed", "3"]
    flagged, plain = tmp_path / "flagged", tmp_path / "plain"
    _run(base + ["--out-dir", str(flagged), "--render-envs", "2", "--render-size", "64x48"], timeout=300)
    _run(base + ["--out-dir", str(plain)], timeout=300)
    s = json.loads((flagged / "eval_summary.json").read_bytes())
    T = s["control_steps"]
    assert T == 8 and s["frames"] == dict(dir="frames", count=2 * T, size=[64, 48], every=1)
    del s["frames"]
    assert (json.dumps(s, indent=1) + "\n").encode() == (plain / "eval_summary.json").read_bytes()
    assert not (plain / "frames").exists()
    for k in range(2):
        files = sorted(p.name for p in (flagged / "frames" / f"env{k:03d}").iterdir())
        assert files == [f"{t:05d}.png" for t in range(T)]
    assert not (flagged / "frames" / "env002").exists()
    frames = np.stack([_decode_png(flagged / "frames" / "env000" / f"{t:05d}.png") for t in range(T)])
    assert frames.shape == (T, 48, 64, 3)
    qpos = np.load(flagged / "trajectory.npz")["qpos"]
    spec = ENVIRONMENTS["jvrc_walk"]()
    rgb, hit, _ = Renderer(spec.model(), 64, 48, device=0).render(qpos[0, 0], aux=True)
    assert np.array_equal(frames[0], rgb[0].cpu().numpy())
    assert (hit[0] >= 0).float().mean().item() >= 0.02      # non-background pixels
    assert not np.array_equal(frames[0], frames[T - 1])      # the robot moved
