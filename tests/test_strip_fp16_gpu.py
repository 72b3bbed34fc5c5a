"""The fp16 strip kernels (csrc/lhw_mlp_strip_h.hip; lhw_ppo_debug_set_strip_fp16, LHW_STRIP_FP16): one forward and one backward launch per
network with fp16 operands, against the per-layer fp16 GEMMs they replace.  The bar everywhere is torch.equal: the strips compute the GEMM
path's accumulator chains on the same MFMA, so no tolerance is involved (the GEMM path itself is pinned to half-rounded references by
tests/test_gemm_gpu.py and tests/test_ppo_gpu.py::test_fp16_*).  Inputs are randn, weights reference_init's: no NaN / inf anywhere.
Kernel against lhw_debug_gemm; two handles (switch on / off) through inference, one minibatch, the plans and the captured step; h1 end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.test_gemm_gpu import _gemm
from tests.test_optimizer_gpu import _ppo_batch
from tests.test_update_plan_gpu import I_GEMM, I_STRIPS, INFER, SWITCHES, U_GEMM, U_TRAIN, UPDATE

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 256
ROWS = (1, 31, 33, 64, 65, 130)      # a lone row, a dead second row tile, a ragged tile, exactly one slab, a slab plus one row, several slabs
WIDTHS = {4: 4, 36: 35, 40: 37, 64: 64}      # Dp: D -- cartpole, h1 (a partial 8-element lane vector), jvrc (a partial 16-k group), the capacity
OUTS = [(1, 4), (10, 12), (12, 12)]
PAD = 3      # sentinel rows behind the R live ones


def _p(t):
    return t.data_ptr() if t is not None else None


def _net(Dp, O, Op, seed):
    """One actor-shaped network in the library's padded layout (pad columns / rows zero), biases non-zero."""
    from learninghumanoidwalking_amd.ppo_kernels import reference_init
    D = WIDTHS.get(Dp, Dp)
    w = reference_init(D, O, H, 0.223, generator_seed=seed)
    g = torch.Generator().manual_seed(seed)
    w1, w3, b3 = torch.zeros(H, Dp), torch.zeros(Op, H), torch.zeros(Op)
    w1[:, :D] = w["a_w1"]
    w3[:O] = w["a_w3"] * 100      # (reference_init scales the actor's read-out by 0.01)
    b3[:O] = 0.1 * torch.randn(O, generator=g)
    b1, b2 = 0.1 * torch.randn(H, generator=g), 0.1 * torch.randn(H, generator=g)
    return {k: v.cuda().contiguous() for k, v in dict(w1=w1, b1=b1, w2=w["a_w2"].clone(), b2=b2, w3=w3, b3=b3).items()}


def _forward_h(n, Dp, O, Op, x, x_half, R, h1, h2, y, hidden=H):
    from learninghumanoidwalking_amd import _lib
    return _lib.lib().lhw_debug_mlp_strip_forward_h(hidden, Dp, O, Op, _p(n["w1"]), _p(n["b1"]), _p(n["w2"]), _p(n["b2"]), _p(n["w3"]), _p(n["b3"]),
                                                    _p(x), x.stride(0), int(x_half), R, _p(h1), _p(h2), _p(y), _p(_scratch()), None)


def _scratch():
    """The debug entries' room for the kernels' fp16 weight copies (sentinel-filled: every half the kernels read is written first)."""
    return torch.full((163840,), float("nan"), device="cuda", dtype=torch.float16)


def _bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("O,Op", OUTS)
@pytest.mark.parametrize("Dp", list(WIDTHS))
def test_forward_strip_is_bit_identical_to_three_fp16_gemm_launches(Dp, O, Op):
    """h1_h, h2_h (as fp16 bits) and y, for every row count and both input forms; rows beyond R (and y's pad columns) keep the sentinel."""
    from learninghumanoidwalking_amd import _lib
    n = _net(Dp, O, Op, seed=Dp + O)
    g = torch.Generator(device="cuda").manual_seed(Dp * 31 + O)
    ldxh = (Dp + 7) // 8 * 8
    for R in ROWS:
        x = torch.randn(R, Dp, device="cuda", generator=g)
        x[:, WIDTHS[Dp]:] = 0
        x_h = torch.zeros(R, ldxh, device="cuda", dtype=torch.float16)
        x_h[:, :Dp] = x.half()
        for x_half, xin in ((0, x), (1, x_h)):
            g1, g2 = (torch.full((R, H), 7.0, device="cuda", dtype=torch.float16) for _ in range(2))
            gy = torch.full((R, Op), 7.0, device="cuda")
            _gemm(True, True, 16 + x_half + 4, R, H, Dp, xin, n["w1"], g1, bias=n["b1"], relu=1)
            _gemm(True, True, 16 + 1 + 4, R, H, H, g1, n["w2"], g2, bias=n["b2"], relu=1)
            _gemm(True, True, 16 + 1, R, O, H, g2, n["w3"], gy, bias=n["b3"])
            h1, h2 = (torch.full((R + PAD, H), 7.0, device="cuda", dtype=torch.float16) for _ in range(2))
            y, y_only = torch.full((R + PAD, Op), 7.0, device="cuda"), torch.full((R + PAD, Op), 7.0, device="cuda")
            _lib.check(_forward_h(n, Dp, O, Op, xin, x_half, R, h1, h2, y))
            _lib.check(_forward_h(n, Dp, O, Op, xin, x_half, R, None, None, y_only))      # (inference: h1 / h2 never leave LDS)
            torch.cuda.synchronize()
            what = (Dp, O, R, x_half)
            assert torch.isfinite(gy[:, :O]).all() and g1.float().abs().sum() > 0 and g2.float().abs().sum() > 0, what
            assert torch.equal(_bits(h1[:R]), _bits(g1)), ("h1", what)
            assert torch.equal(_bits(h2[:R]), _bits(g2)), ("h2", what)
            assert torch.equal(y[:R], gy) and torch.equal(y_only, y), ("y", what)
            assert (h1[R:] == 7.0).all() and (h2[R:] == 7.0).all() and (y[R:] == 7.0).all() and (y[:, O:] == 7.0).all(), ("sentinel", what)


@pytest.mark.parametrize("O,Op", OUTS)
def test_backward_strip_is_bit_identical_to_two_fp16_gemm_launches(O, Op):
    """dh2_h and dh1_h as fp16 bits: dy float32 rounded while staged, the masks read from the stored fp16 activations."""
    from learninghumanoidwalking_amd import _lib
    L = _lib.lib()
    n = _net(40, O, Op, seed=50 + O)
    g = torch.Generator(device="cuda").manual_seed(7 + O)
    for R in ROWS:
        dy = torch.randn(R, Op, device="cuda", generator=g)
        h1, h2 = (torch.relu(torch.randn(R, H, device="cuda", generator=g)).half() for _ in range(2))      # half the units off, as after a ReLU
        g2, g1 = (torch.full((R, H), 7.0, device="cuda", dtype=torch.float16) for _ in range(2))
        _gemm(True, False, 16 + 4 + 8, R, H, O, dy, n["w3"], g2, mask=h2)
        _gemm(True, False, 16 + 1 + 4 + 8, R, H, H, g2, n["w2"], g1, mask=h1)
        dh2, dh1 = (torch.full((R + PAD, H), 7.0, device="cuda", dtype=torch.float16) for _ in range(2))
        _lib.check(L.lhw_debug_mlp_strip_backward_h(H, O, Op, _p(n["w2"]), _p(n["w3"]), _p(dy), R, _p(h1), _p(h2), _p(dh2), _p(dh1), _p(_scratch()), None))
        torch.cuda.synchronize()
        assert g2.float().abs().sum() > 0 and g1.float().abs().sum() > 0 and torch.isfinite(g1.float()).all(), (O, R)
        assert torch.equal(_bits(dh2[:R]), _bits(g2)), ("dh2", O, R)
        assert torch.equal(_bits(dh1[:R]), _bits(g1)), ("dh1", O, R)
        assert (dh2[R:] == 7.0).all() and (dh1[R:] == 7.0).all(), ("sentinel", O, R)


@pytest.mark.parametrize("hidden,Dp", [(256, 68), (128, 40)])
def test_unsupported_shapes_are_refused_with_nothing_written(hidden, Dp):
    from learninghumanoidwalking_amd import _lib
    L = _lib.lib()
    R, O, Op = 33, 12, 12
    n = {k: torch.zeros(256 * 256, device="cuda") for k in ("w1", "b1", "w2", "b2", "w3", "b3")}
    x = torch.randn(R, Dp, device="cuda")
    h1, h2 = (torch.full((R, 256), 7.0, device="cuda", dtype=torch.float16) for _ in range(2))
    y = torch.full((R, Op), 7.0, device="cuda")
    assert _forward_h(n, Dp, O, Op, x, 0, R, h1, h2, y, hidden=hidden) == -4      # LHW_ERR_UNSUPPORTED
    if hidden != 256:
        dy = torch.randn(R, Op, device="cuda")
        assert L.lhw_debug_mlp_strip_backward_h(hidden, O, Op, _p(n["w2"]), _p(n["w3"]), _p(dy), R, _p(h1), _p(h2), _p(h1), _p(h2), _p(_scratch()), None) == -4
    torch.cuda.synchronize()
    assert (h1 == 7.0).all() and (h2 == 7.0).all() and (y == 7.0).all()


# ---------------------------------------------------------------------------------------------------------------- through a handle
D, A, CAP = 37, 12, 130


def _handle(monkeypatch, strip_fp16, env=None, **kw):
    """obs 37 (40 padded columns), 12 actions, 130 rows, a signed permutation as mirror tables; the switch is set on the handle itself."""
    from learninghumanoidwalking_amd.ppo_kernels import PpoKernels, reference_init
    for name in SWITCHES + ("LHW_STRIP_FP16",):
        monkeypatch.delenv(name, raising=False)
    for name, value in (env or {}).items():
        monkeypatch.setenv(name, value)
    rs = np.random.default_rng(99)
    mir = dict(mirror_obs=(rs.permutation(D).astype(np.int32), rs.choice([-1.0, 1.0], size=D).astype(np.float32)),
               mirror_act=(rs.permutation(A).astype(np.int32), rs.choice([-1.0, 1.0], size=A).astype(np.float32)))
    k = PpoKernels(D, A, hidden=256, max_rows=CAP, **{"lr": 1e-3, "learn_std": True, "entropy_coeff": 0.01, **mir, **kw})
    k.set_tensors(reference_init(D, A, 256, 0.223, generator_seed=7))
    k.set_obs_norm(rs.normal(size=D).astype(np.float32) * 0.1, (0.5 + rs.uniform(size=D)).astype(np.float32))
    k.set_strip_fp16(strip_fp16)
    return k


def _plan(k):
    plan = k.plan(k.max_rows)
    return {f: plan[f] for f in UPDATE}, {f: plan[f] for f in INFER}


def test_plans_report_the_fp16_strips_only_where_they_run(monkeypatch):
    on = _handle(monkeypatch, True)
    assert _plan(on) == (U_TRAIN, I_STRIPS), "float32 dtypes: today's plans"
    on.set_update_fp16(True)
    on.set_inference_fp16(True)
    u, i = _plan(on)
    assert u == dict(U_GEMM, fp16_operands=1, fp16_storage=1, fwd_strip=3, bwd_strip=3)      # no train strips, no mask bits, not wide
    assert i == dict(I_STRIPS, infer_fp16_operands=1, infer_strips=1, policy_step=0)
    off = _handle(monkeypatch, False)
    off.set_update_fp16(True)
    off.set_inference_fp16(True)
    assert _plan(off) == (dict(U_GEMM, fp16_operands=1, fp16_storage=1), dict(I_STRIPS, infer_fp16_operands=1, infer_strips=0, policy_step=0))
    f32_storage = _handle(monkeypatch, True, env=dict(LHW_FP16_STORAGE="0"))
    f32_storage.set_update_fp16(True)
    assert _plan(f32_storage) == (dict(U_GEMM, fp16_operands=1), I_STRIPS), "float32-stored activations keep the GEMMs"
    no_strips = _handle(monkeypatch, True, env=dict(LHW_MLP_STRIP="0"))
    no_strips.set_update_fp16(True)
    no_strips.set_inference_fp16(True)
    assert _plan(no_strips) == (dict(U_GEMM, fp16_operands=1, fp16_storage=1), dict(I_GEMM, infer_fp16_operands=1))
    from learninghumanoidwalking_amd.ppo_kernels import PpoKernels
    wide = PpoKernels(111, A, hidden=256, max_rows=64)      # rows of 112 columns: outside the fp16 strips' shapes, the GEMMs stay
    wide.set_strip_fp16(True)
    wide.set_update_fp16(True)
    assert {f: wide.plan(64)[f] for f in UPDATE} == dict(U_GEMM, fp16_operands=1, fp16_storage=1)


def test_fp16_inference_is_the_same_bits_with_the_switch_on_and_off(monkeypatch):
    """PpoKernels.forward of 130 rows and of 33 rows at workspace row 65: mu, the value, the action and its log-density."""
    ks = {sw: _handle(monkeypatch, sw) for sw in (False, True)}
    obs = torch.randn(CAP, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))
    res = {}
    for sw, k in ks.items():
        k.set_inference_fp16(True)
        assert k.plan()["infer_strips"] == int(sw)
        full = k.forward(obs, seed=5, env_id_base=17, counter=9)
        part = k.forward(obs[40:73], seed=5, env_id_base=3, counter=2, ws_row=65)
        torch.cuda.synchronize()
        res[sw] = [t.clone() for t in full + part]
    assert torch.isfinite(res[False][0]).all() and res[False][0].abs().sum() > 0
    for a, b, name in zip(res[False], res[True], ("mu", "act", "logp", "value") * 2):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("B", [CAP, 70])      # the actor's 2 B rows as one span / as two spans (the mirrored rows from row 130)
def test_fp16_minibatch_gradient_is_the_same_bits_with_the_switch_on_and_off(B, monkeypatch):
    ks = {sw: _handle(monkeypatch, sw) for sw in (False, True)}
    for k in ks.values():
        k.set_update_fp16(True)
    rs = np.random.default_rng(B)
    xn, xm, act, logp, adv, ret, idx = _ppo_batch(ks[False], rs, 2 * CAP, 1, B)
    logp = logp + torch.tensor(rs.uniform(-0.5, 0.5, size=2 * CAP).astype(np.float32)).cuda()      # ratios on both sides of the clip range
    for sw, k in ks.items():
        k.grad_minibatch(xn, xm, act, logp, adv, ret, idx[0])
        torch.cuda.synchronize()
        assert k.last_grad_fused == 0 and k.plan(B)["fwd_strip"] == k.plan(B)["bwd_strip"] == (3 if sw else 0)
    ref, got = ks[False], ks[True]
    assert torch.isfinite(ref.grad).all() and ref.grad.abs().sum() > 0 and 0 < float(ref.stats[4]) < 1, "clip fraction strictly between 0 and 1"
    assert torch.equal(ref.grad, got.grad), "flat gradient"
    assert torch.equal(ref.stats[:6], got.stats[:6]), "loss statistics"


def test_toggling_the_switch_recaptures_the_step(monkeypatch):
    """lhw_ppo_step with the switch on, off, on == a second handle that made the same calls eagerly: the captured step's key holds the plan."""
    B = 64
    graph, eager = _handle(monkeypatch, False), _handle(monkeypatch, False)
    for k in (graph, eager):
        k.set_update_fp16(True)
    rs = np.random.default_rng(5)
    stream = torch.cuda.Stream()      # not the legacy default stream: that one cannot be captured
    with torch.cuda.stream(stream):
        xn, xm, act, logp, adv, ret, idx = _ppo_batch(graph, rs, 2 * CAP, 3, B)
        for t, on in enumerate((1, 0, 1)):
            for k in (graph, eager):
                k.set_strip_fp16(on)
            graph.step_minibatch(xn, xm, act, logp, adv, ret, idx[t])
            eager.grad_minibatch(xn, xm, act, logp, adv, ret, idx[t])
            eager.apply()
            stream.synchronize()
            for k in (graph, eager):
                assert k.plan(B)["fwd_strip"] == 3 * on and k.plan(B)["train_strip"] == 0
    for name in ("theta", "adam_m", "adam_v"):
        assert torch.equal(getattr(graph, name), getattr(eager, name)), name
    assert torch.equal(graph.stats[:6], eager.stats[:6])


# ---------------------------------------------------------------------------------------------------------------- end to end
_CHILD = r"""
import sys, torch
from types import SimpleNamespace
sys.path.insert(0, sys.argv[1])
from learninghumanoidwalking_amd.envs import ENVIRONMENTS
from learninghumanoidwalking_amd.ppo import PPO
out, mode, N, T = sys.argv[2], sys.argv[3], 64, 8
a = SimpleNamespace(gamma=0.99, lam=0.95, lr=3e-4, eps=1e-5, entropy_coeff=0.0, clip=0.2, minibatch_size=N * T // 2, epochs=1, max_traj_len=T,
                    num_procs=N, num_envs=N, max_grad_norm=0.5, mirror_coeff=0.4, eval_freq=10**9, recurrent=False, imitate=None,
                    learn_std=False, std_dev=0.4, no_mirror=False, continued=None, logdir=out + "_log", device_index=0,
                    fp16=mode == "fp16", infer_fp16=mode == "infer")
algo = PPO(ENVIRONMENTS["h1"], a, seed=9)
res = {}
for it in range(2):
    algo.sample_parallel_with_workers()
    ro = algo.rollout
    for n in ("obs", "act", "logp", "tob_all", "rew", "done", "val", "vterm", "vfinal"):
        res[f"{n}{it}"] = getattr(ro, n).cpu().clone()
    algo.optimize(it)
    torch.cuda.synchronize()
    res[f"theta{it}"] = algo.kernels.theta.cpu().clone()
res["plan"] = algo.kernels.plan()
res["mode"] = ro.last_mode
torch.save(res, out)
"""


@pytest.mark.parametrize("mode,rollout", [("fp16", "auto"), ("infer", "steps")])
def test_two_iterations_of_h1_are_the_same_bits_with_the_fp16_strips(mode, rollout, tmp_path):
    """h1, 64 envs, T = 8, two iterations, same seed, under LHW_STRIP_FP16=1 and unset, each in a fresh child process (PpoKernels reads the
    variable when the handle is made): --fp16, and --infer-fp16 alone with the launch-per-step rollout (lhw_ppo_forward_at is what runs)."""
    script = tmp_path / "child.py"
    script.write_text(_CHILD)
    res = {}
    for sw in ("1", None):
        out = tmp_path / f"strip_fp16_{sw}.pt"
        env = {k: v for k, v in os.environ.items() if k not in SWITCHES + ("LHW_STRIP_FP16",)}
        env["LHW_ROLLOUT_MODE"] = rollout
        if sw:
            env["LHW_STRIP_FP16"] = sw
        r = subprocess.run([sys.executable, str(script), ROOT, str(out), mode], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        res[sw] = torch.load(out)
    on, off = res["1"]["plan"], res[None]["plan"]
    assert on["infer_fp16_operands"] == off["infer_fp16_operands"] == 1 and on["infer_strips"] == 1 and off["infer_strips"] == 0
    if mode == "fp16":
        assert on["fwd_strip"] == on["bwd_strip"] == 3 and off["fwd_strip"] == off["bwd_strip"] == 0 and on["fp16_storage"] == off["fp16_storage"] == 1
    else:
        assert res["1"]["mode"] == res[None]["mode"] == "steps"
    keys = [k for k in res["1"] if k not in ("plan", "mode")]
    assert len(keys) == 20
    for key in keys:
        assert torch.equal(res["1"][key], res[None][key]), key
    assert not torch.equal(res["1"]["theta0"], res["1"]["theta1"])
