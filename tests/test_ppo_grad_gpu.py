"""What lhw_ppo_grad leaves in ``grad`` and ``stats[:6]`` against float64 autograd (tests/ppo_grad_reference.py): one grad_minibatch on a zeroed
gradient, no apply().  The post-Adam comparisons of tests/test_ppo_gpu.py see a relative gradient error d only as lr / 4 * d in a weight; here every
tensor of the gradient is compared directly, per kernel path, with the path asserted from the handle's plan.

Per case: the plan is the one the case is written for; every tensor within bar(P) = 8 x max(y(P), median y of its network), y the distance of the
SAME reference evaluated in float32 on the CPU from the float64 one (never a figure taken from the kernels); exact zeros where the float64
gradient is identically zero and at every padding element of the flat vector; the loss scalars likewise (clip_fraction 1e-6); every negative
control of the reference (critic gradient x 0.5, PPO term x 1.01, mirror mean over B, clipped rows let through, entropy coefficient x 2, imitation
denominator B k, the twin's gradient dropped) rejected by >= 10 bars wherever its term is active.  Inputs: target ratios {0.5 .. 2.0} on both sides
of and inside the clip range through old_logp = logp64 - log(target) (no row within 1e-3 of an edge), advantages of both signs and exact zeros,
>= 2 rows of every class asserted, unequal stds 0.15 .. 0.4, non-zero biases, the actor read-out not scaled down, a non-trivial observation
normalisation, idx a scrambled subset of the stored rows.

The loss scalars are means of per-row terms whose float32 errors cancel: |s32 - s64| of one evaluation is one draw of that sum, so a scalar's
yardstick is the larger of the draw and the scale it is drawn from (ppo_grad_reference.scalar_bars).  The draw alone is unsound as a yardstick: the
reference itself in float32 with its sums in another order misses 8 x it on the CPU
(tests/test_grad_reference.py::test_another_summation_order_stays_within_the_bars).  Each reported scalar taken 1 % too large must lie >= 10 bars off.

Measured on an MI355X, worst error / y per path over its cases: first with y floored by its network's median, as in the bar (the bar is 8;
nothing above 4), then over each tensor's OWN y(P), which the bar does not use alone:
    train strips (12 shape / mirror / std variants)      3.79  c_b3, B = 256 mirror on (the others 1.5 .. 2.2)    own y 6.49  c_b3
    forward strip, loss kernel, backward strip           1.73  stds, 48 rows without mask bits; 1.62 with them    own y 3.21  stds
    imitation armed                                      2.09  approx_kl                                          own y 1.64  c_b1
    per-layer GEMMs, LHW_MLP_STRIP=0                     3.08  stds                                               own y 3.08  stds
    per-layer GEMMs, hidden 64                           2.63  c_b3, B = 33 mirror off                            own y 38.7  c_b3, B = 256 mirror off
    D = 35, A = 10                                       1.83  c_w1 (hidden 256); 2.10 a_w2 (hidden 64)           own y 2.36  stds
    wide rows D = 111, strips / GEMMs                    2.41  a_w1 (the same bits on both)                       own y 2.41  a_w1
    one stream                                           2.09  approx_kl                                          own y 1.64  c_b1
    two calls accumulating                               2.16  a_b3                                               own y 2.16  a_b3
Own y above 4 only on c_b3: the critic's read-out bias is ONE number, so its y is one draw of float32 roundoff (7.7e-9 in the CPU case of
tests/test_grad_reference.py, against 2e-7 on its neighbours) -- what the median in the bar is there for; its error is at most 0.5 bars.
Negative controls, the smallest rejection over all cases, in bars: critic x 0.5 1.6e5, PPO term x 1.01 490, mirror mean over B 3.3e4, no min
2.6e4, entropy coefficient x 2 47.6, imitation denominator 4.6e3, twin's gradient dropped 1.8e3; a reported scalar x 1.01: 15.7 (actor_loss).
"""
import numpy as np
import pytest
import torch

from tests import ppo_grad_reference as R
from tests.test_optimizer_gpu import PAD_A, PAD_D, PAD_MIR_ACT, PAD_MIR_OBS
from tests.test_ppo_gpu import MIR_ACT, MIR_OBS
from tests.test_update_plan_gpu import U_GEMM, U_STRIPS, U_TRAIN, UPDATE, _call, _handle

pytestmark = pytest.mark.gpu

ENTROPY = 0.01


def _case(B, max_rows, plan, *, mirror=False, learn_std=False, env=None, calls=(), hidden=256, D=37, A=12, imitation=False):
    return dict(B=B, max_rows=max_rows, plan=plan, mirror=mirror, learn_std=learn_std, env=env or {}, calls=list(calls), hidden=hidden, D=D, A=A,
                imitation=imitation)


CASES = {}
for _B, _cap in ((33, 64), (200, 256), (256, 256)):
    for _m in (False, True):
        for _s in (False, True):
            CASES[f"train-B{_B}of{_cap}-{'mirror' if _m else 'nomirror'}-{'std' if _s else 'fixedstd'}"] = _case(_B, _cap, U_TRAIN, mirror=_m, learn_std=_s)
CASES.update({
    # forward strip, loss kernel, backward strip: with the mask bits (capacity a multiple of 64) and without
    "fused-off-B256-bits": _case(256, 256, U_STRIPS, mirror=True, learn_std=True, calls=[("fused", 0)]),
    "fused-off-48-rows": _case(48, 48, dict(U_STRIPS, mask_bits=0), mirror=True, learn_std=True, calls=[("fused", 0)]),
    # an armed imitation term (3 of 12 action columns, about half the rows) takes the strips and the loss kernel
    "imitation-B200": _case(200, 256, U_STRIPS, mirror=True, imitation=True),
    "gemm-strip0-B200": _case(200, 256, U_GEMM, mirror=True, learn_std=True, env=dict(LHW_MLP_STRIP="0")),
    "gemm-h64-B33-mirror": _case(33, 64, U_GEMM, mirror=True, hidden=64),
    "gemm-h64-B33-nomirror": _case(33, 64, U_GEMM, hidden=64),
    "gemm-h64-B256-mirror": _case(256, 256, U_GEMM, mirror=True, hidden=64),
    "gemm-h64-B256-nomirror": _case(256, 256, U_GEMM, hidden=64),
    # D = 35, A = 10: every kind of padding exists
    "pad-35x10-h256": _case(33, 64, U_TRAIN, mirror=True, learn_std=True, D=PAD_D, A=PAD_A),
    "pad-35x10-h64": _case(33, 64, U_GEMM, mirror=True, learn_std=True, D=PAD_D, A=PAD_A, hidden=64),
    "wide-111-strips": _case(33, 64, dict(U_TRAIN, wide=1), learn_std=True, D=111, calls=[("wide", 1)]),
    "wide-111-gemm": _case(33, 64, U_GEMM, learn_std=True, D=111, calls=[("wide", 0)]),
    "one-stream-B200": _case(200, 256, dict(U_TRAIN, streams=1), mirror=True, env=dict(LHW_PPO_TWO_STREAMS="0")),
})


def _setup(c, monkeypatch, n_minibatches=1):
    """The handle of case c with the test's weights, and stored rows for n_minibatches disjoint scrambled minibatches of B rows."""
    from oracle import ppo_oracle as po
    D, A, H, B = c["D"], c["A"], c["hidden"], c["B"]
    kw = {}
    if c["mirror"]:
        mo, ma = (po.mirror_tables(MIR_OBS, [29, 30]), po.mirror_tables(MIR_ACT)) if D == 37 else (po.mirror_tables(PAD_MIR_OBS), po.mirror_tables(PAD_MIR_ACT))
        kw = dict(mirror_obs=mo, mirror_act=ma)
    k = _handle(monkeypatch, c["env"], obs_dim=D, hidden=H, max_rows=c["max_rows"], act_dim=A, learn_std=c["learn_std"],
                entropy_coeff=ENTROPY if c["learn_std"] else 0.0, **kw)
    for what, on in c["calls"]:
        _call(k, what, on)
    rs = np.random.default_rng(1000 * B + D + H + c["mirror"] + 2 * c["learn_std"])
    w = k.get_tensors()
    for n in w:      # (reference_init: unit-norm rows, zero biases, the actor read-out x 0.01)
        if n.endswith(("b1", "b2", "b3")):
            w[n] = torch.tensor(rs.normal(size=tuple(w[n].shape)).astype(np.float32) * 0.1)
    w["a_w3"] = w["a_w3"] * 100.0
    w["stds"] = torch.tensor(np.linspace(0.15, 0.4, A).astype(np.float32))
    k.set_tensors(w)
    mean, std = rs.normal(size=D).astype(np.float32) * 0.3, (0.5 + rs.uniform(size=D)).astype(np.float32)
    k.set_obs_norm(mean, std)
    rows = n_minibatches * B + 31
    obs = torch.tensor(rs.normal(size=(rows, D)).astype(np.float32) * std + mean).cuda()
    xn, xm = k.normalize(obs)
    assert not xn[:, D:].any() and (xm is None or not xm[:, D:].any())
    perm = rs.permutation(rows)
    mbs = [perm[i * B:(i + 1) * B] for i in range(n_minibatches)]
    theta = {n: t.numpy() for n, t in k.get_tensors().items()}
    xn_h, xm_h = xn[:, :D].cpu().numpy(), (xm[:, :D].cpu().numpy() if c["mirror"] else None)
    act, old_logp, adv, ret = R.ff_inputs(theta, xn_h, mbs, rs)
    imits = [None] * n_minibatches
    if c["imitation"]:
        imits = []
        for _ in mbs:
            mask = torch.zeros(B, A, dtype=torch.uint8)
            mask[torch.tensor(rs.uniform(size=B) < 0.5)[:, None] & torch.isin(torch.arange(A), torch.tensor([0, 2, 5]))[None, :]] = 1
            imits.append((0.5, torch.tensor(rs.normal(size=(B, A)).astype(np.float32)), mask, int(mask.sum())))
    dev = dict(xn=xn, xm=xm if c["mirror"] else None, act=act.cuda(), old_logp=old_logp.cuda(), adv=adv.cuda(), ret=ret.cuda())

    def ref_of(i):
        idx = mbs[i]
        kwr = dict(entropy_coeff=ENTROPY if c["learn_std"] else 0.0, learn_std=c["learn_std"], mirror_act=kw.get("mirror_act"), imitation=imits[i])
        return lambda **o: R.ff_reference(theta, xn_h[idx], None if xm_h is None else xm_h[idx], act[idx], old_logp[idx], adv[idx], ret[idx], **kwr, **o)

    def run(i):
        im = imits[i]
        k.grad_minibatch(dev["xn"], dev["xm"], dev["act"], dev["old_logp"], dev["adv"], dev["ret"], torch.tensor(mbs[i].astype(np.int32)).cuda(),
                         imitation=None if im is None else (im[0], im[1].cuda(), im[2].cuda(), im[3]))
    return k, run, ref_of, adv, mbs


def _active(c):
    return dict(mirror=c["mirror"], learn_std=c["learn_std"], imitation=c["imitation"])


@pytest.mark.parametrize("case", list(CASES))
def test_minibatch_gradient_matches_float64_autograd(case, monkeypatch):
    c = CASES[case]
    k, run, ref_of, adv, mbs = _setup(c, monkeypatch)
    plan = k.plan(c["B"], c["imitation"])
    assert {f: plan[f] for f in UPDATE} == c["plan"], "the handle plans the path this case is written for"
    ref = ref_of(0)
    R.assert_classes(case, ref(want_rows=True)[2]["ratio"], adv[mbs[0]].numpy())
    k.grad.zero_()
    k.stats.zero_()
    run(0)
    torch.cuda.synchronize()
    assert k.last_grad_fused == c["plan"]["train_strip"], "and that path ran"
    R.check_gradient(case, k, ref, R.FF_MUTATIONS, _active(c))


def test_two_calls_accumulate_the_sum_of_two_minibatches(monkeypatch):
    """lhw_ppo_grad "accumulates into grad and stats_dev[0..5]": two calls on two different idx without apply() leave the sum of the two
    references (train strips, mirror on, learnable stds: the std slots take two column sums and two entropy terms)."""
    c = CASES["train-B33of64-mirror-std"]
    k, run, ref_of, adv, mbs = _setup(c, monkeypatch, n_minibatches=2)
    plan = k.plan(c["B"], False)
    assert {f: plan[f] for f in UPDATE} == c["plan"]
    for i in (0, 1):
        R.assert_classes(f"accumulate-ff minibatch {i}", ref_of(i)(want_rows=True)[2]["ratio"], adv[mbs[i]].numpy())
    k.grad.zero_()
    k.stats.zero_()
    for i in (0, 1):
        run(i)
        torch.cuda.synchronize()
        assert k.last_grad_fused == c["plan"]["train_strip"]

    def both(**o):
        a, b = ref_of(0)(**o), ref_of(1)(**o)
        out = (a[0] + b[0], {n: a[1][n] + b[1][n] for n in a[1]})
        # (with want_rows: the sum of two means over M rows each is the mean of the 2 M doubled terms)
        return out + ({i: 2.0 * np.concatenate([a[2][i], b[2][i]]) for i in a[2]},) if len(a) == 3 else out
    R.check_gradient("accumulate-ff", k, both, R.FF_MUTATIONS, _active(c))
