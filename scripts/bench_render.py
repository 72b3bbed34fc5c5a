"""Cost of an eval frame: milliseconds of lhw_render_frames per 640 x 480 frame of the jvrc_walk scene, per-tile culling on and off (shadows
on), and the host's PNG-encoding time per frame.  HIP events around LAUNCHES calls of FRAMES frames each on poses uploaded beforehand, the
two settings alternating, after a warm-up of each.

    python scripts/bench_render.py [--frames 64] [--launches 50] [--repeats 5] [--size 640x480] [--env jvrc_walk]
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from learninghumanoidwalking_amd.envs import ENVIRONMENTS      # noqa: E402
from learninghumanoidwalking_amd.kinematics import body_poses, geom_poses      # noqa: E402
from learninghumanoidwalking_amd.render import Renderer, TrackingCamera, write_png      # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--frames", type=int, default=64)
    p.add_argument("--launches", type=int, default=50)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--size", default="640x480")
    p.add_argument("--env", default="jvrc_walk")
    a = p.parse_args()
    W, H = (int(x) for x in a.size.split("x"))
    spec = ENVIRONMENTS[a.env]()
    m = spec.model()
    rng = np.random.default_rng(0)
    q = np.tile(spec.nominal_pose, (a.frames, 1))
    q[:, 0] += 0.02 * np.arange(a.frames)                      # the robot walks through the checkerboard
    q[:, 7:] += 0.1 * rng.normal(size=(a.frames, m.nq - 7))
    t0 = time.perf_counter()
    pos, mat = geom_poses(m, q)
    cam_pos, cam_rows = TrackingCamera().poses(body_poses(m, q)[0])
    t_kin = (time.perf_counter() - t0) * 1e3 / a.frames
    print(f"{a.env}: {m.ngeom} geoms, {W} x {H}, shadows on, {a.launches} launches of {a.frames} frames per timed window, {torch.cuda.get_device_name(0)}")
    rs = {cull: Renderer(m, W, H, device=0, cull=cull) for cull in (True, False)}
    frames = rs[True].upload(pos, mat, cam_pos, cam_rows)
    rgb = {cull: torch.empty(a.frames, H, W, 3, dtype=torch.uint8, device="cuda") for cull in rs}
    for cull, r in rs.items():
        r.draw(frames, rgb[cull])                               # warm-up: the first launch loads the code object
    torch.cuda.synchronize()
    assert torch.equal(rgb[True], rgb[False])
    ms = {True: [], False: []}
    for _ in range(a.repeats):
        for cull, r in rs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                r.draw(frames, rgb[cull])
            e1.record()
            torch.cuda.synchronize()
            ms[cull].append(e0.elapsed_time(e1) / (a.launches * a.frames))
    for cull in (True, False):
        v = np.array(ms[cull])
        print(f"cull {'on ' if cull else 'off'}: {np.median(v):.4f} ms / frame (min {v.min():.4f}, max {v.max():.4f} over {a.repeats} windows of "
              f"{v.mean() * a.launches * a.frames:.0f} ms; a call reads its three geom tables back before it launches, which is in the figure)")
    host = rgb[True].cpu().numpy()
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        for f in range(a.frames):
            write_png(os.path.join(d, "frame.png"), host[f])
        dt = (time.perf_counter() - t0) * 1e3 / a.frames
        size = os.path.getsize(os.path.join(d, "frame.png"))
    print(f"host: write_png {dt:.2f} ms / frame (zlib level 6, {size} bytes), kinematics + camera {t_kin:.3f} ms / frame")


if __name__ == "__main__":
    main()
