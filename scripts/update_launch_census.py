"""Launch census of one feed-forward PPO handle, for comparing two trees kernel by kernel.

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python scripts/update_launch_census.py CASE
  python scripts/update_launch_census.py --table OUT/.../*_kernel_trace.csv

CASE names one setting of the handle's switches, dtypes, shape and row capacity (the table of tests/test_update_plan_gpu.py).  The run, all on
min(64, max_rows) rows: create the handle; one forward for actions + log-densities, one for values only; begin_rollout / rollout_policy /
end_rollout; one eager grad_minibatch + apply; two step_minibatch on a side stream.  It uses only PpoKernels calls older trees have too, so
the same file runs against either tree (the package is the working directory's).  --table prints, per kernel name, the multiset of (grid, workgroup)
sizes of a kernel trace: two trees launch the same kernels exactly when their tables are equal."""
import collections
import csv
import os
import sys

# CASE: (environment, PpoKernels arguments, calls on the new handle, imitation term armed for the eager minibatch)
CASES = {
    "default": ({}, {}, [], False),
    "fused-off": ({}, {}, [("fused", 0)], False),
    "fused-off-48-rows": ({}, dict(max_rows=48), [("fused", 0)], False),
    "bits-off": (dict(LHW_STRIP_BITS="0"), {}, [("fused", 0)], False),
    "imitation-armed": ({}, {}, [], True),
    "update-fp16": ({}, {}, [("update_fp16", 1)], False),
    "update-fp16-f32-storage": (dict(LHW_FP16_STORAGE="0"), {}, [("update_fp16", 1)], False),
    "inference-fp16": ({}, {}, [("inference_fp16", 1)], False),
    "mlp-strip-1": (dict(LHW_MLP_STRIP="1"), {}, [], False),
    "mlp-strip-0": (dict(LHW_MLP_STRIP="0"), {}, [], False),
    "obs-111-wide-off": ({}, dict(obs_dim=111), [], False),
    "obs-111-wide-on": ({}, dict(obs_dim=111), [("wide", 1)], False),
    "hidden-64": ({}, dict(hidden=64), [], False),
    "one-stream": (dict(LHW_PPO_TWO_STREAMS="0"), {}, [], False),
}
SWITCHES = ("LHW_MLP_STRIP", "LHW_STRIP_BITS", "LHW_STRIP_FUSED", "LHW_STRIP_WIDE", "LHW_STRIP_FP16", "LHW_PPO_TWO_STREAMS", "LHW_PPO_GRAPH", "LHW_FP16_STORAGE")
ACT = 12


def run(case):
    env, kw, calls, imitation = CASES[case]
    for name in SWITCHES:      # before the package loads the library: some trees read a switch once per process
        os.environ.pop(name, None)
    os.environ.update(env)
    sys.path.insert(0, os.getcwd())
    import numpy as np
    import torch
    from learninghumanoidwalking_amd import _lib
    from learninghumanoidwalking_amd.ppo_kernels import PpoKernels, reference_init

    kw = dict(dict(obs_dim=37, hidden=256, max_rows=64), **kw)
    k = PpoKernels(kw["obs_dim"], ACT, hidden=kw["hidden"], max_rows=kw["max_rows"], lr=1e-3)
    k.set_tensors(reference_init(kw["obs_dim"], ACT, kw["hidden"], 0.223, generator_seed=7))
    for what, on in calls:
        if what == "fused":
            _lib.check(k._L.lhw_ppo_debug_set_strip_fused(k._h, on))
        elif what == "wide":
            _lib.check(k._L.lhw_ppo_debug_set_strip_wide(k._h, on))
        elif what == "update_fp16":
            k.set_update_fp16(bool(on))
        else:
            k.set_inference_fp16(bool(on))
    B = min(64, k.max_rows)
    rs = np.random.default_rng(3)
    obs = torch.tensor(rs.normal(size=(B, k.obs_dim)).astype(np.float32)).cuda()
    _, act, logp, _ = k.forward(obs, seed=5, want_value=False, want_mu=False)
    k.forward(obs, want_actor=False)
    k.begin_rollout()
    view = k.rollout_policy()
    k.end_rollout()
    adv = torch.tensor(rs.normal(size=B).astype(np.float32)).cuda()
    ret = torch.tensor(rs.normal(size=B).astype(np.float32)).cuda()
    xn, _ = k.normalize(obs, want_mirror=False)
    idx = [torch.tensor(rs.permutation(B).astype(np.int32)).cuda() for _ in range(3)]
    imit = None
    if imitation:
        mask = torch.tensor(rs.integers(0, 2, size=(B, ACT)).astype(np.uint8)).cuda()
        imit = (0.5, torch.zeros(B, ACT, device="cuda"), mask, max(int(mask.sum()), 1))
    k.grad_minibatch(xn, None, act, logp, adv, ret, idx[0], imitation=imit)
    fused = [k.last_grad_fused]
    k.apply()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        for t in (1, 2):
            k.step_minibatch(xn, None, act, logp, adv, ret, idx[t])
        fused.append(k.last_grad_fused)
        stream.synchronize()
    torch.cuda.synchronize()
    print(f"census {case}: rows {B} rollout_policy {'view' if view is not None else 'None'}"
          f"{' fp16_operands' if view is not None and view.fp16_operands else ''} last_grad_fused eager {fused[0]} step {fused[1]}"
          f" theta_sum {float(k.theta.double().sum()):.17g}")


def table(path):
    rows = collections.Counter()
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows[(r["Kernel_Name"], tuple(int(r[f"Grid_Size_{a}"]) for a in "XYZ"), tuple(int(r[f"Workgroup_Size_{a}"]) for a in "XYZ"))] += 1
    for (name, grid, wg), n in sorted(rows.items()):
        print(f"{n:4d} x grid {grid} workgroup {wg}  {name}")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--table":
        table(sys.argv[2])
    elif len(sys.argv) == 2 and sys.argv[1] in CASES:
        run(sys.argv[1])
    else:
        sys.exit(f"usage: {sys.argv[0]} CASE | --table KERNEL_TRACE.csv\ncases: {' '.join(CASES)}")
