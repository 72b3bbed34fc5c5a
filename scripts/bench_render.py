"""Cost of an eval frame: milliseconds of lhw_render_frames per 640 x 480 frame of the jvrc_walk scene, per-tile culling on and off (shadows
on), and the host's PNG-encoding time per frame.  HIP events around LAUNCHES calls of FRAMES frames each on poses uploaded beforehand, the
two settings alternating, after a warm-up of each.

    python scripts/bench_render.py [--frames 64] [--launches 50] [--repeats 5] [--size 640x480] [--env jvrc_walk]

`--scene`: the cost of lhw_render_scene instead -- three cases alternating in one run: lhw_render_frames on the jvrc_walk scene, lhw_render_scene
on the same scene without a dynamic geom, lhw_render_scene on a full jvrc_step frame (the model, the 21 terrain geoms of markers.step_terrain
and the markers of a 20-step sequence from markers.step_markers) -- and the PNG encoding of that last frame on the host.

    python scripts/bench_render.py --scene [--frames 64] [--launches 20] [--repeats 5] [--size 640x480]
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


def stepping_scene(frames):
    """(renderer arguments of) a full jvrc_step frame: the robot walking up a staircase of 20 footsteps, terrain and every marker drawn"""
    from learninghumanoidwalking_amd import _lib, markers as M
    spec = ENVIRONMENTS["jvrc_step"]()
    m = spec.model()
    q = np.tile(spec.nominal_pose, (frames, 1))
    q[:, 0] += 0.02 * np.arange(frames)
    seq = np.zeros((frames, 20, 4))
    seq[:, :, 0], seq[:, :, 1], seq[:, :, 2] = 0.35 * np.arange(20), 0.1 * (-1.0) ** np.arange(20), 0.05 * np.arange(20)
    nseq = np.full(frames, 20)
    xpos = body_poses(m, q)[0]
    stin = np.zeros((frames, _lib.STEP_TASK_INPUT_DIM))
    S = _lib.STEP_TASK_INPUT_FIELDS
    rfoot, lfoot = spec.body_ids()[2:4]
    stin[:, S["rsite_xpos"][0]:S["rsite_xpos"][0] + 3], stin[:, S["lsite_xpos"][0]:S["lsite_xpos"][0] + 3] = xpos[:, rfoot], xpos[:, lfoot]
    stin[:, S["t1"][0]], stin[:, S["t2"][0]], stin[:, S["nseq"][0]] = 1, 2, 20
    box0, floor = spec.terrain_ids()
    box_h = np.asarray(m.arrays["geom_size"]).reshape(-1, 3)[box0:box0 + M.NBOX, 2]
    dyn = M.step_terrain(seq, nseq, np.zeros(frames), box_h).merge(M.step_markers(np.zeros((frames, _lib.TASK_INPUT_DIM)), stin, seq, nseq, m, q, (rfoot, lfoot)))
    return m, q, list(range(box0, box0 + M.NBOX)) + [floor], dyn.arrays(frames)


def scene_bench(a, W, H):
    walk = ENVIRONMENTS["jvrc_walk"]()
    mw = walk.model()
    qw = np.tile(walk.nominal_pose, (a.frames, 1))
    qw[:, 0] += 0.02 * np.arange(a.frames)
    ms_, qs, hidden, dyn = stepping_scene(a.frames)
    rw, rs = Renderer(mw, W, H, device=0), Renderer(ms_, W, H, device=0, hidden_geoms=hidden)

    def uploads(r, m, q, d):
        pos, mat = geom_poses(m, q)
        cam_pos, cam_rows = TrackingCamera().poses(body_poses(m, q)[0])
        return r.upload(pos, mat, cam_pos, cam_rows), r.upload_dynamic(d, cam_pos)

    empty = dict(type=np.zeros((a.frames, 0), np.int32))
    fw, dw = uploads(rw, mw, qw, empty)
    fs, ds = uploads(rs, ms_, qs, dyn)
    rgb = torch.empty(a.frames, H, W, 3, dtype=torch.uint8, device="cuda")
    cases = {"lhw_render_frames, jvrc_walk (9 geoms)": lambda: rw.draw(fw, rgb),
             "lhw_render_scene,  jvrc_walk (9 + 0 geoms)": lambda: rw.draw_scene(fw, dw, rgb),
             f"lhw_render_scene,  jvrc_step ({rs.n_geoms} + {ds[0].shape[1]} geoms, terrain and markers)": lambda: rs.draw_scene(fs, ds, rgb)}
    print(f"{W} x {H}, shadows on, culling on, {a.launches} launches of {a.frames} frames per timed window, {torch.cuda.get_device_name(0)}")
    for fn in cases.values():
        fn()                                                    # warm-up: the first launch loads the code object
    torch.cuda.synchronize()
    ms = {k: [] for k in cases}
    for _ in range(a.repeats):
        for k, fn in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / (a.launches * a.frames))
    for k, v in ms.items():
        v = np.array(v)
        print(f"{k}: {np.median(v):.4f} ms / frame (min {v.min():.4f}, max {v.max():.4f} over {a.repeats} windows; the table read-back of a call is in the figure)")
    host = rgb.cpu().numpy()                                    # (the last case drawn: the stepping frames)
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        for f in range(a.frames):
            write_png(os.path.join(d, "frame.png"), host[f])
        dt = (time.perf_counter() - t0) * 1e3 / a.frames
    step_ms = float(np.median(ms[list(cases)[2]]))
    print(f"host: write_png of a jvrc_step frame {dt:.2f} ms / frame; the frame costs {step_ms:.4f} ms on the device: {'below' if step_ms < dt else 'NOT below'} its encoding")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--scene", action="store_true", help="lhw_render_scene: frames entry, scene entry on the same scene, a full jvrc_step frame")
    p.add_argument("--frames", type=int, default=64)
    p.add_argument("--launches", type=int, default=50)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--size", default="640x480")
    p.add_argument("--env", default="jvrc_walk")
    a = p.parse_args()
    W, H = (int(x) for x in a.size.split("x"))
    if a.scene:
        return scene_bench(a, W, H)
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
