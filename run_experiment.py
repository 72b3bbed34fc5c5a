"""Entry point with the reference's `train` and `eval` command lines (reference run_experiment.py:153-208, 245-292), running the
on-device rollout + PPO of this repository.

    python run_experiment.py train --env jvrc_walk --logdir /tmp/logs --num-envs 4096 --n-itr 100 --seed 0
    python run_experiment.py train --env jvrc_walk --gpus 8 ...        (re-executes itself as 8 ranks under torch.distributed.run)
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 run_experiment.py train --env jvrc_walk ...
    python run_experiment.py eval --path RUN_DIR|ACTOR.pt [--num-envs 64] [--ep-len 10] [--seed S] [--out-dir DIR] [--trace-envs 16]
    python run_experiment.py eval --path RUN_DIR --out-dir DIR --render-envs 2 [--render-size 640x480] [--render-every 1] [--render-markers]
    python run_experiment.py eval --path RUN_DIR --out-dir DIR --render-envs 2 --render-format mjpeg [--render-quality 90]     (DIR/video/env000.avi)
    python run_experiment.py eval --path RUN_DIR --command forward:0.1..0.4 [--num-envs 4]     (walking tasks: pinned commands)
    python run_experiment.py eval --path RUN_DIR --footsteps forward:0.0..0.1 [--num-envs 4]   (jvrc_step: pinned walk modes / footstep plans)
    python run_experiment.py eval --logdir DIR ...                     (latest run below DIR, its latest actor)

Differences from the reference, by design: no Ray (`--num-procs` is the number of on-device envs per GPU unless
`--num-envs` is given); with `--recurrent` (LSTM actor / critic) `--minibatch-size` counts env columns = trajectories, as it
counts trajectories in the reference; `--imitate` needs an env description with `imitation_projector()` (as in the reference).
`train --term-stats` also writes <run dir>/reward_terms.csv, one row per iteration with the mean episode sum of every reward term (the
`info` dictionaries of the reference's env.step, accumulated inside the stepping kernels).

`eval` is headless (the reference's opens a GL viewer on CPU MuJoCo, run_experiment.py:277-292: not part of this repository): it runs
`--num-envs` deterministic episodes of `--ep-len` seconds in parallel on the device, prints one JSON object -- checkpoint, env, seed,
episodes, terminated, truncated, mean return, mean length, mean episode sum per reward term -- and writes it to eval_summary.json in
`--out-dir` (default: the run directory).  With `--out-dir`, a feed-forward policy also leaves trajectory.npz there: qpos [T][K][nq],
qvel, action, reward, done and the task-input record task_inputs [T][K][176] of the first `--trace-envs` envs -- on jvrc_step also
step_task_inputs [T][K][32] and the terrain in force during every control step, terrain_seq [T][K][20][4] (x y z theta of every footstep /
box), terrain_nseq, terrain_floor_z -- enough to replay the motion in a MuJoCo viewer elsewhere.  `--render-envs K` also draws the first K
of them, one PNG per control step under DIR/frames/env<k>/ -- the tracking camera of the reference's eval (rl/utils/eval.py:38-67) through
the HIP ray caster of render.py, no GL and no MuJoCo; jvrc_step with its terrain boxes -- and adds "frames" to the summary.
`--render-markers` draws the task's markers into them (the reference's draw_markers: velocity arrows, footstep targets, foot frames).
`--render-format mjpeg` (or `both`) delivers the frames as the reference's eval does, as a video: DIR/video/env<k>.avi, Motion-JPEG in AVI
at real-time speed, every frame coded on the device right behind the ray caster (video.py: lhw_jpeg_encode, `--render-quality`) so that
only compressed bytes reach the host; the summary gains "video".
`--command SPEC` (jvrc_walk, h1_walk) pins every env's command before the reset the episodes start from, instead of the task's draw --
standing | inplace:YAW | forward:VX[,VY], a value A..B spread linearly over the envs -- and adds "command" and "per_env" (mode, mode_ref,
return and length of each env's first episode) to the summary: one launch gives a return-against-commanded-speed curve.
`--footsteps SPEC` (jvrc_step) does the same for the stepping task, whose command is a walk mode and a footstep plan: forward[:H] (H the
rise per step, A..B spread over the envs) | backward | standing | lateral[:left|right] | curved[:K] | plan:FILE[:K] (FILE in the format of
the env's plans file, an optional fourth column z) -- and adds "footsteps", "per_env" (mode, height, nseq, return, length and
targets_reached of each env's first episode) and the fault counters "contact_overflow" / "diverged" to the summary: one launch says how
high a stair the policy climbs, or whether it follows the plan it is given.
"""
import argparse
import json
import math
import os
import pickle
import shutil
import sys
from datetime import datetime
from functools import partial
from pathlib import Path


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--env", required=True, type=str)
    p.add_argument("--logdir", default=Path("/tmp/logs"), type=Path)
    p.add_argument("--input-norm-steps", type=int, default=100000)
    p.add_argument("--n-itr", type=int, default=20000)
    p.add_argument("--lr", type=float, default=3e-4)
    p.add_argument("--eps", type=float, default=1e-5)
    p.add_argument("--gamma", type=float, default=0.99)
    p.add_argument("--lam", type=float, default=0.95)
    p.add_argument("--std-dev", type=float, default=0.223)
    p.add_argument("--learn-std", action="store_true")
    p.add_argument("--entropy-coeff", type=float, default=0.0)
    p.add_argument("--clip", type=float, default=0.2)
    p.add_argument("--minibatch-size", type=int, default=64)
    p.add_argument("--epochs", type=int, default=3)
    p.add_argument("--num-procs", type=int, default=12)
    p.add_argument("--num-envs", type=int, default=None, help="on-device environments per GPU (default: --num-procs)")
    p.add_argument("--max-grad-norm", type=float, default=0.5)
    p.add_argument("--max-traj-len", type=int, default=400)
    p.add_argument("--no-mirror", action="store_true")
    p.add_argument("--mirror-coeff", default=0.4, type=float)
    p.add_argument("--eval-freq", default=100, type=int)
    p.add_argument("--continued", type=Path)
    p.add_argument("--recurrent", action="store_true")
    p.add_argument("--imitate", type=str, default=None)
    p.add_argument("--infer-fp16", action="store_true", help="rollout inference with fp16 operands (update stays float32)")
    p.add_argument("--fp16", action="store_true", help="fp16 actor / critic: inference and all GEMMs of the update with fp16 operands, float32 accumulation / master weights / Adam")
    p.add_argument("--imitate-coeff", type=float, default=0.3)
    p.add_argument("--yaml", type=str, default=None)
    p.add_argument("--device", type=str, default="auto", choices=["auto", "cpu", "cuda"])
    p.add_argument("--seed", type=int, default=None)
    p.add_argument("--term-stats", dest="term_stats", action=argparse.BooleanOptionalAction, default=None,
                   help="per-term episode reward statistics from the stepping kernels, logged to reward_terms.csv (default: off; -0.6 % env-steps/s on jvrc_walk @ 4096)")
    p.add_argument("--gpus", type=int, default=1, help="GPUs of this node to train on (data parallel: envs sharded, gradients all-reduced over RCCL); "
                                                        "N > 1 outside a torch.distributed.run launcher re-executes this command as N ranks")
    return p


def run_experiment(args):
    import torch
    import torch.distributed as dist
    from learninghumanoidwalking_amd.envs import ENVIRONMENTS
    from learninghumanoidwalking_amd.ppo import PPO

    if args.device == "cpu" or not torch.cuda.is_available():
        raise SystemExit("this trainer runs on MI355X only: there is no CPU path (use the reference for --device cpu)")
    world = int(os.environ.get("WORLD_SIZE", 1))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    share = os.environ.get("LHW_SHARE_GPU") == "1"     # (tests only: every rank on GPU 0 over gloo, to run the N > 1 path on a 1-GPU box)
    if share:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if share:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    rank = dist.get_rank() if world > 1 else 0
    if args.env not in ENVIRONMENTS:
        raise SystemExit(f"unknown --env {args.env!r}; available: {sorted(ENVIRONMENTS)}")
    stamp = [datetime.now().strftime("%y-%m-%d-%H-%M-%S-%f")[:-3]]
    if world > 1:
        dist.broadcast_object_list(stamp, src=0)     # one log directory per run, named by rank 0's clock
    args.logdir = Path(args.logdir) / f"{stamp[0]}_{args.env}"
    args.device_index = local_rank
    Spec = ENVIRONMENTS[args.env]
    env_fn = partial(Spec, yaml_path=args.yaml) if (args.yaml and args.env != "cartpole") else Spec
    if rank == 0:
        Path.mkdir(args.logdir, parents=True, exist_ok=True)
        with open(Path(args.logdir, "experiment.pkl"), "wb") as f:   # run_experiment.py:136-139
            pickle.dump(args, f)
        if args.yaml:
            shutil.copyfile(args.yaml, Path(args.logdir, "config.yaml"))
    if args.seed is not None:
        torch.manual_seed(args.seed)
    algo = PPO(env_fn, args, seed=args.seed)
    algo.train(env_fn, args.n_itr)
    if world > 1:
        dist.destroy_process_group()


def build_eval_parser():
    p = argparse.ArgumentParser(prog="run_experiment.py eval")
    p.add_argument("--path", type=Path, default=None, help="an actor checkpoint (.pt) or a run directory (its latest actor)")
    p.add_argument("--logdir", type=Path, default=None, help="a directory of runs: the latest run, its latest actor")
    p.add_argument("--num-envs", type=int, default=64, help="episodes run in parallel")
    p.add_argument("--ep-len", type=float, default=10.0, help="episode length in seconds")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--out-dir", type=Path, default=None, help="where eval_summary.json (and trajectory.npz) go; default: the run directory, summary only")
    p.add_argument("--trace-envs", type=int, default=16, help="envs whose trajectory is written with --out-dir")
    p.add_argument("--render-envs", type=int, default=0, help="with --out-dir: PNG frames of the first K traced envs, frames/env<k>/<step>.png (0: none, no renderer is created)")
    p.add_argument("--render-size", type=_size, default=(640, 480), metavar="WxH", help="frame size in pixels (the reference's eval: 640x480)")
    p.add_argument("--render-every", type=int, default=1, metavar="N", help="a frame every N control steps")
    p.add_argument("--render-format", choices=("png", "mjpeg", "both"), default="png", help="png: frames/env<k>/<step>.png; mjpeg: video/env<k>.avi, Motion-JPEG coded on the device; both")
    p.add_argument("--render-quality", type=int, default=90, metavar="Q", help="JPEG quality 1..100 of --render-format mjpeg")
    p.add_argument("--render-markers", action="store_true", help="draw the task's markers into the frames: velocity arrows (walking tasks), footstep targets and foot frames (jvrc_step)")
    p.add_argument("--command", type=str, default=None, metavar="SPEC",
                   help="walking tasks: pin every env's command instead of drawing it: standing | inplace:YAW | forward:VX[,VY]; a value A..B is spread linearly over the envs")
    p.add_argument("--footsteps", type=str, default=None, metavar="SPEC",
                   help=f"jvrc_step: pin every env's walk mode and footstep plan instead of drawing them: {FOOTSTEP_FORMS}; H may be A..B, spread linearly over the envs")
    return p


COMMAND_ENVS = ("jvrc_walk", "h1_walk")      # the envs whose command can be pinned (BatchedEnv.pin_commands)


def parse_command(text, K):
    """`eval --command SPEC` for K envs -> (mode [K] int32, mode_ref [K][3] float64 = yaw rate, forward speed, lateral speed).
    SPEC: standing | inplace:YAW | forward:VX[,VY]; a value may be A..B, spread linearly over the envs: env k gets A + k (B - A) / (K - 1),
    and K = 1 gets A."""
    import numpy as np

    def spread(v):
        try:
            a, b = (float(x) for x in v.split("..")) if ".." in v else (float(v), float(v))
        except ValueError:
            raise SystemExit(f"eval: --command {text!r}: {v!r} is neither a number nor A..B") from None
        if not (math.isfinite(a) and math.isfinite(b)):
            raise SystemExit(f"eval: --command {text!r}: {v!r} is not finite")
        return np.array([a + k * (b - a) / (K - 1) if K > 1 else a for k in range(K)], dtype=np.float64)

    name, _, rest = text.partition(":")
    vals = [v for v in rest.split(",")] if rest else []
    want = {"standing": (0, 0), "inplace": (1, 1), "forward": (1, 2)}
    if name not in want or not want[name][0] <= len(vals) <= want[name][1] or any(not v.strip() for v in vals):
        raise SystemExit(f"eval: --command {text!r} is none of standing | inplace:YAW | forward:VX[,VY]")
    mode = ("standing", "inplace", "forward").index(name)
    ref = np.zeros((K, 3))
    if name == "inplace":
        ref[:, 0] = spread(vals[0].strip())
    elif name == "forward":
        ref[:, 1] = spread(vals[0].strip())
        if len(vals) == 2:
            ref[:, 2] = spread(vals[1].strip())
    return np.full(K, mode, dtype=np.int32), ref


FOOTSTEP_FORMS = "forward[:H] | backward | standing | lateral[:left|right] | curved[:K] | plan:FILE[:K]"


def parse_footsteps(text, K, nplans):
    """`eval --footsteps SPEC` (jvrc_step) for K envs of an env whose plan table has `nplans` rows -> the per-env pin fields, the keywords
    of BatchedEnv.pin_step_plans: dict(mode [K] int32, choice [K] int32 (-1: drawn), height [K] float64 (NaN: the stair schedule's),
    steps: a list of K plans [n][4] = x, y, z, theta, or None where every env's sequence is generated).
    SPEC: forward[:H] (H the signed rise per step; A..B is spread linearly over the envs as parse_command spreads) | backward | standing |
    lateral[:left|right] | curved[:K] (a row of the env's plan table) | plan:FILE[:K] (FILE as load_plans reads it -- plans closed by
    `---`, rows `x,y,theta` with an optional fourth column z -- of 2..20 steps each; without K env k walks plan k mod their number; a
    plan with some z != 0 is walked in FORWARD mode, which sinks the floor under the stairs, else in CURVED mode)."""
    import numpy as np
    from learninghumanoidwalking_amd._lib import STEP_COMMAND_MODES, STEP_MAX_SEQ
    from learninghumanoidwalking_amd.envs.jvrc_step import load_plans

    def fail(why):
        raise SystemExit(f"eval: --footsteps {text!r}: {why}") from None

    def index(v, n, what):
        if not v.isdigit() or int(v) >= n:
            fail(f"{v!r} is not one of the {n} {what} (0..{n - 1})")
        return int(v)

    name, _, rest = text.partition(":")
    if name not in STEP_COMMAND_MODES + ("plan",) or (":" in text and not rest) or (rest and name in ("backward", "standing")):
        fail(f"is none of {FOOTSTEP_FORMS}")
    out = dict(mode=np.full(K, STEP_COMMAND_MODES.index(name) if name != "plan" else 0, dtype=np.int32), choice=np.full(K, -1, dtype=np.int32),
               height=np.full(K, np.nan), steps=None)
    if name == "forward" and rest:
        try:
            a, b = (float(x) for x in rest.split("..")) if ".." in rest else (float(rest), float(rest))
        except ValueError:
            fail(f"{rest!r} is neither a number nor A..B")
        if not (math.isfinite(a) and math.isfinite(b)):
            fail(f"{rest!r} is not finite")
        out["height"][:] = [a + k * (b - a) / (K - 1) if K > 1 else a for k in range(K)]
    elif name == "lateral" and rest:
        if rest not in ("left", "right"):
            fail(f"{rest!r} is neither left nor right")
        out["choice"][:] = 1 if rest == "left" else 0      # (the task's draw 0 gives sign -1: steps towards -y, the robot's right)
    elif name == "curved" and rest:
        out["choice"][:] = index(rest, nplans, "plans of the env's table")
    elif name == "plan":
        path, _, tail = rest.rpartition(":")
        path, tail = (path, tail) if path and tail.isdigit() else (rest, "")
        try:
            plans = load_plans(path)
        except OSError as e:
            fail(f"cannot read {path!r} ({e.strerror})")
        except ValueError as e:
            if "could not convert" in str(e):
                fail(f"{path!r} holds a row that is not numbers separated by commas")
            fail(f"{path!r} holds a plan whose rows differ in their number of columns (every row of a plan has 3, x,y,theta, or 4, x,y,theta,z)")
        if not plans:
            fail(f"{path!r} holds no plan (every plan is closed by a line `---`)")
        for i, p in enumerate(plans):
            if p.ndim != 2 or p.shape[1] not in (3, 4) or not np.isfinite(p).all():
                fail(f"plan {i} of {path!r} must have rows of 3 (x,y,theta) or 4 (x,y,theta,z) finite numbers")
            if not 2 <= len(p) <= STEP_MAX_SEQ:
                fail(f"plan {i} of {path!r} has {len(p)} steps (2..{STEP_MAX_SEQ} supported)")
        # the file's columns x, y, theta [, z] -> the pin's x, y, z, theta
        plans = [np.column_stack([p[:, 0], p[:, 1], p[:, 3] if p.shape[1] == 4 else np.zeros(len(p)), p[:, 2]]) for p in plans]
        pick = [index(tail, len(plans), f"plans of {path!r}")] * K if tail else [k % len(plans) for k in range(K)]
        out["steps"] = [plans[i] for i in pick]
        out["mode"][:] = [STEP_COMMAND_MODES.index("forward" if plans[i][:, 2].any() else "curved") for i in pick]
    return out


def first_episodes(rew, done):
    """(return [K] float64, length [K]) of every env's first episode from the rollout's rew [T][K] / done [T][K]: the rewards up to and
    including the first step whose done flag is set (the whole rollout if none is), summed in float64 in time order."""
    import numpy as np
    rew, done = np.asarray(rew, dtype=np.float64), np.asarray(done)
    T, K = rew.shape
    ret, length = np.zeros(K), np.zeros(K, dtype=np.int64)
    for k in range(K):
        ended = np.flatnonzero(done[:, k] != 0)
        length[k] = int(ended[0]) + 1 if ended.size else T
        for t in range(length[k]):
            ret[k] += rew[t, k]
    return ret, length


def _size(text):
    try:
        w, h = (int(x) for x in text.lower().split("x"))
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r} is not WxH") from None
    if w < 1 or h < 1:
        raise argparse.ArgumentTypeError(f"{text!r}: both sizes must be at least 1")
    return w, h


def write_frames(out_dir, env, spec, record, size, every, markers=False, fmt="png", quality=90):
    """PNG frames of the traced motion, the tracking camera of the reference's eval (rl/utils/eval.py:38-67) on every env:
    <out_dir>/frames/env<k:03d>/<t:05d>.png for every `every`-th control step t.  `record`: the arrays of trajectory.npz -- qpos [T][K][nq],
    task_inputs [T][K][176] and, on jvrc_step, step_task_inputs and terrain_seq / _nseq / _floor_z, from which the terrain of every frame is
    drawn (markers.step_terrain in place of the model's own boxes and floor).  `markers`: also the task's markers (markers.walk_markers /
    step_markers; a task without a command -- h1 standing -- has none).  `fmt` "mjpeg" / "both": the same frames as <out_dir>/video/env<k:03d>.avi,
    coded chunk by chunk on the device (video.JpegEncoder at `quality`) and played at 1 / (control_dt * every) frames a second; "mjpeg" writes
    no PNG.  Returns the summary's ("frames", "video") entries, None for the one not written."""
    import numpy as np
    from learninghumanoidwalking_amd import markers as M
    from learninghumanoidwalking_amd.render import Renderer, write_png
    png, avi = fmt in ("png", "both"), fmt in ("mjpeg", "both")
    hidden, entry = (), dict(dir="frames", count=0, size=list(size), every=every)
    qpos = record["qpos"]
    stepping = "terrain_seq" in record
    if stepping:
        box0, floor = spec.terrain_ids()
        hidden = list(range(box0, box0 + M.NBOX)) + [floor]
        box_h = np.asarray(env.model.arrays["geom_size"]).reshape(-1, 3)[box0:box0 + M.NBOX, 2]
    elif getattr(spec, "name", "") == "jvrc_step":      # (an LSTM policy's rollout keeps no terrain record: the boxes stay hidden)
        hidden = list(range(spec.terrain_ids()[0], spec.terrain_ids()[0] + M.NBOX))
        entry["note"] = "the stepping terrain's boxes are not drawn: a recurrent policy's rollout does not record their poses"
    walking = markers and getattr(spec, "name", "") in ("jvrc_walk", "h1_walk")
    if markers:
        entry["markers"] = True
    r = Renderer(env.model, size[0], size[1], device=env.device, hidden_geoms=hidden)
    steps = list(range(0, qpos.shape[0], every))
    video = None
    if avi:
        from learninghumanoidwalking_amd.video import JpegEncoder, MjpegWriter
        enc = JpegEncoder(size[0], size[1], quality, device=env.device)
        video = dict(dir="video", count=qpos.shape[1], frames=len(steps), size=list(size), every=every, fps=1.0 / (float(record["control_dt"]) * every), quality=quality)
        Path(out_dir, "video").mkdir(parents=True, exist_ok=True)
    for k in range(qpos.shape[1]):
        d = Path(out_dir, "frames", f"env{k:03d}")
        if png:
            d.mkdir(parents=True, exist_ok=True)
        writer = MjpegWriter(Path(out_dir, "video", f"env{k:03d}.avi"), size[0], size[1], video["fps"]) if avi else None
        for i in range(0, len(steps), r.frames_per_chunk):
            part = steps[i:i + r.frames_per_chunk]
            dyn = None
            if stepping:
                seq, nseq = record["terrain_seq"][part, k], record["terrain_nseq"][part, k]
                dyn = M.step_terrain(seq, nseq, record["terrain_floor_z"][part, k], box_h, env.model.geom_rgba[floor] if env.model.geom_rgba is not None else (0.5, 0.5, 0.5, 1.0))
                if markers:
                    dyn.merge(M.step_markers(record["task_inputs"][part, k], record["step_task_inputs"][part, k], seq, nseq, env.model, qpos[part, k], spec.body_ids()[2:4]))
            elif walking:
                dyn = M.walk_markers(record["task_inputs"][part, k])
            rgb = r.render(qpos[part, k], markers=dyn)
            if avi:      # (the chunk is coded where it was drawn: only the compressed bytes are copied)
                for data in enc.encode(rgb):
                    writer.add(data)
            if png:
                for t, img in zip(part, rgb.cpu().numpy()):
                    write_png(d / f"{t:05d}.png", img)
                entry["count"] += len(part)
        if avi:
            writer.close()
    return (entry if png else None), video


def get_latest_actor(run_dir: Path) -> Path:
    """The checkpoint of the highest iteration, actor_<itr>.pt, else actor.pt (the best one)."""
    numbered = [(int(f.stem.split("_")[1]), f) for f in Path(run_dir).glob("actor_*.pt") if f.stem.split("_")[1].isdigit()]
    if numbered:
        return max(numbered)[1]
    if Path(run_dir, "actor.pt").is_file():
        return Path(run_dir, "actor.pt")
    raise SystemExit(f"eval: no actor checkpoint (actor_<itr>.pt / actor.pt) in {run_dir}")


def get_latest_run(logdir: Path) -> Path:
    """The newest run directory below `logdir` (run directories start with their time stamp, so the names sort by age)."""
    runs = sorted(d for d in Path(logdir).iterdir() if d.is_dir() and Path(d, "experiment.pkl").is_file()) if Path(logdir).is_dir() else []
    if not runs:
        raise SystemExit(f"eval: no run directory (one holding experiment.pkl) in {logdir}")
    return runs[-1]


def resolve_checkpoint(path, logdir):
    """(actor.pt, critic.pt, experiment.pkl) as the reference resolves them (run_experiment.py:245-269): --path names an actor file
    or a run directory, --logdir a directory of runs; the critic and the pickled training arguments lie beside the actor."""
    if (path is None) == (logdir is None):
        raise SystemExit("eval: give exactly one of --path ACTOR.pt|RUN_DIR and --logdir DIR")
    if logdir is not None:
        path = get_latest_run(logdir)
    path = Path(path)
    if path.is_dir():
        actor = get_latest_actor(path)
    elif path.is_file() and path.suffix == ".pt" and path.name.startswith("actor"):
        actor = path
    else:
        raise SystemExit(f"eval: {path} is neither an actor checkpoint (actor*.pt) nor a run directory")
    critic = actor.with_name("critic" + actor.name[len("actor"):])
    pkl = actor.with_name("experiment.pkl")
    for f in (critic, pkl):
        if not f.is_file():
            raise SystemExit(f"eval: {f} is missing (it must lie beside {actor.name})")
    return actor, critic, pkl


def run_eval(argv):
    ea = build_eval_parser().parse_args(argv)
    if ea.render_envs > 0 and ea.out_dir is None:
        raise SystemExit("eval: --render-envs needs --out-dir (the frames go to <out-dir>/frames)")
    if ea.render_envs < 0 or ea.render_every < 1:
        raise SystemExit("eval: --render-envs must be >= 0 and --render-every >= 1")
    if not 1 <= ea.render_quality <= 100:
        raise SystemExit("eval: --render-quality must lie in 1..100")
    actor, critic, pkl = resolve_checkpoint(ea.path, ea.logdir)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("this trainer runs on MI355X only: there is no CPU path (use the reference for --device cpu)")
    import numpy as np
    from learninghumanoidwalking_amd import _lib
    from learninghumanoidwalking_amd.envs import ENVIRONMENTS
    from learninghumanoidwalking_amd.ppo import PPO
    with open(pkl, "rb") as f:
        args = pickle.load(f)
    if args.env not in ENVIRONMENTS:
        raise SystemExit(f"eval: unknown env {args.env!r} in {pkl}")
    if ea.command is not None and args.env not in COMMAND_ENVS:
        raise SystemExit(f"eval: --command pins the command of a walking task ({', '.join(COMMAND_ENVS)}); the env of this run, {args.env}, has none to pin")
    if ea.footsteps is not None and args.env != "jvrc_step":
        raise SystemExit(f"eval: --footsteps pins the footstep plan of the stepping task (jvrc_step); the env of this run, {args.env}, has none to pin")
    Spec = ENVIRONMENTS[args.env]
    yaml = Path(actor.parent, "config.yaml")      # the run's own copy of --yaml (run_experiment.py train)
    env_fn = partial(Spec, yaml_path=str(yaml)) if (yaml.is_file() and args.env != "cartpole") else Spec
    T = int(math.ceil(ea.ep_len / env_fn().control_dt - 1e-9))
    out_dir = ea.out_dir if ea.out_dir is not None else actor.parent
    Path(out_dir).mkdir(parents=True, exist_ok=True)
    # the learner of `train`, loaded like --continued (checkpoint.py's loaders, the checkpoint's observation normalisation), on a batch of
    # its own: T control steps with max_traj_len = T, so every env finishes exactly one counted episode -- it falls, or it is truncated
    # at the horizon -- and whatever a reset starts after a fall is cut by the horizon and not counted
    args.continued, args.logdir, args.device_index = actor, out_dir, 0
    args.num_envs, args.max_traj_len, args.imitate, args.gpus = ea.num_envs, T, None, 1
    args.minibatch_size = min(int(args.minibatch_size or ea.num_envs), ea.num_envs) if getattr(args, "recurrent", False) else args.minibatch_size
    torch.cuda.set_device(0)
    torch.manual_seed(ea.seed)
    algo = PPO(env_fn, args, seed=ea.seed, term_stats=True)
    if ea.out_dir is not None:
        algo.rollout.record_task_inputs = True      # (kept by the resident rollout; asking for it selects that path for an LSTM actor too)
        if args.env == "jvrc_step" and hasattr(algo.rollout, "record_terrain"):
            algo.rollout.record_terrain = True      # launch per step, bitwise the resident rollout: the terrain of every control step is read on the way
    if ea.command is not None:
        # every env is pinned BEFORE the reset whose observation the rollout starts from: that observation carries the command
        mode, ref = parse_command(ea.command, ea.num_envs)
        algo.env.pin_commands(mode, ref)
        algo.rollout.started = False      # (the rollout resets the env before its first control step)
    if ea.footsteps is not None:
        # likewise: the reset the rollout starts from already lays out the pinned plan
        pins = parse_footsteps(ea.footsteps, ea.num_envs, len(algo.spec.plans))
        algo.env.pin_step_plans(pins["mode"], height=pins["height"], choice=pins["choice"], steps=pins["steps"])
        algo.env.pop_fault_stats()
        algo.rollout.record_task_inputs = True      # (the stepping record of every control step: targets_reached below)
        algo.rollout.started = False
    algo.sample_parallel_with_workers(deterministic=True)      # Rollout.collect(deterministic=True), as PPO.evaluate
    ls = algo._ep_stats[1]
    ts = algo.term_stats
    # (the return is the sum of its terms; the term sums are added up in env order, whereas the env's own return counter is a float atomic
    # whose last bits follow the order in which wavefronts finish: the same command twice must write the same bytes)
    summary = dict(checkpoint=str(actor), env=args.env, seed=ea.seed, num_envs=ea.num_envs, control_steps=T, episodes=ts["episodes"],
                   terminated=ts["terminated"], truncated=ts["truncated"], mean_return=sum(ts["terms"].values()) if ts["episodes"] else float("nan"),
                   mean_length=ls / ts["episodes"] if ts["episodes"] else float("nan"), terms=ts["terms"])
    if ea.command is not None:
        # one launch, a return-against-command curve: every env's command and the return / length of the episode it started with
        ret, length = first_episodes(algo.rollout.rew.cpu().numpy(), algo.rollout.done.cpu().numpy())
        summary["command"] = ea.command
        summary["per_env"] = [dict(mode=int(mode[k]), mode_ref=[float(x) for x in ref[k]], episode_return=float(ret[k]), episode_length=int(length[k]))
                              for k in range(ea.num_envs)]
    if ea.footsteps is not None:
        # per env, the plan it was given and how far it got: the targets it reached are the largest t1 its first episode's record shows
        ret, length = first_episodes(algo.rollout.rew.cpu().numpy(), algo.rollout.done.cpu().numpy())
        stin = getattr(algo.rollout, "stin_all", None)
        t1 = None if stin is None else stin[:, :, _lib.STEP_TASK_INPUT_FIELDS["t1"][0]].cpu().numpy()
        summary["footsteps"] = ea.footsteps
        summary["per_env"] = [dict(mode=_lib.STEP_COMMAND_MODES[int(pins["mode"][k])], height=None if math.isnan(pins["height"][k]) else float(pins["height"][k]),
                                   nseq=0 if pins["steps"] is None else len(pins["steps"][k]), **{"return": float(ret[k])}, length=int(length[k]),
                                   targets_reached=None if t1 is None else int(t1[:length[k], k].max()))
                              for k in range(ea.num_envs)]
        # (a plan can stack more boxes under a foot than the contact merge holds: the control steps that dropped contacts, and the diverged ones)
        summary["contact_overflow"], summary["diverged"] = algo.env.pop_fault_stats()
        if t1 is None:
            summary["targets_reached"] = f"not reported: the rollout ({getattr(algo.rollout, 'last_mode', None)}) kept no stepping record of its control steps"
    if ea.out_dir is not None:
        if algo.rollout.tin_all is None:
            summary["trajectory"] = f"not written: the rollout ran launch-per-step ({algo.rollout.last_mode}), which keeps no per-step record"
            if ea.render_envs > 0:
                summary.update({k: summary["trajectory"] for k, fmts in (("frames", ("png", "both")), ("video", ("mjpeg", "both"))) if ea.render_format in fmts})
        else:
            ro, K = algo.rollout, max(1, min(ea.trace_envs, ea.num_envs))
            rec = ro.tin_all[:, :K].cpu().numpy()
            pad = np.ones(rec.shape[-1], dtype=bool)      # (the record's pad columns are written by nobody: zero in the file)
            for o, n in _lib.TASK_INPUT_FIELDS.values():
                pad[o:o + n] = False
            rec[:, :, pad] = 0.0
            q0, v0, a0 = (_lib.TASK_INPUT_FIELDS[k][0] for k in ("qpos", "qvel", "action"))
            env = algo.env
            record = dict(qpos=rec[:, :, q0:q0 + env.nq], qvel=rec[:, :, v0:v0 + env.nv], action=rec[:, :, a0:a0 + env.act_dim],
                          reward=ro.rew[:, :K].cpu().numpy(), done=ro.done[:, :K].cpu().numpy(), control_dt=np.float64(env_fn().control_dt), task_inputs=rec)
            if getattr(ro, "last_mode", None) == "recorded":      # jvrc_step: what a replay of the episode needs beyond the robot's state
                record.update(step_task_inputs=ro.stin_all[:, :K].cpu().numpy(), terrain_seq=ro.terrain_seq[:, :K], terrain_nseq=ro.terrain_nseq[:, :K],
                              terrain_floor_z=ro.terrain_floor_z[:, :K])
            np.savez(Path(out_dir, "trajectory.npz"), **record)
            summary["trajectory"] = "trajectory.npz"
            if ea.render_envs > 0:
                R = min(ea.render_envs, K)
                frames, video = write_frames(out_dir, env, algo.spec, {k: (v[:, :R] if np.ndim(v) >= 2 else v) for k, v in record.items()}, ea.render_size,
                                             ea.render_every, markers=ea.render_markers, fmt=ea.render_format, quality=ea.render_quality)
                summary.update({k: v for k, v in (("frames", frames), ("video", video)) if v is not None})
    text = json.dumps(summary, indent=1)
    with open(Path(out_dir, "eval_summary.json"), "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] not in ("train", "eval"):
        raise SystemExit("usage: run_experiment.py train --env <name> [...] | run_experiment.py eval (--path ACTOR.pt|RUN_DIR | --logdir DIR) [...]")
    if sys.argv[1] == "eval":
        run_eval(sys.argv[2:])
        sys.exit(0)
    sys.argv.remove("train")
    args = build_parser().parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        from learninghumanoidwalking_amd.dist_utils import relaunch_under_torchrun
        raise SystemExit(relaunch_under_torchrun(args.gpus, os.path.abspath(__file__), ["train"] + sys.argv[1:]))
    run_experiment(args)
