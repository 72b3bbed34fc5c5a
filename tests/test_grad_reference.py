"""tests/ppo_grad_reference.py (the float64 autograd reference of the PPO minibatch gradient) against the CPU oracle, which the fixtures pin to
the reference project: with max_grad_norm large enough that nothing is clipped, ``.grad`` after OraclePPO.update / OracleRecurrentPPO.update is
the raw autograd gradient of a float32 evaluation.  Bar: the float32 yardstick's own distance to the float64 gradient times MARGIN, as for the
kernels.  And: each negative-control mutation changes the reference gradient by at least 1e-3 relative (max-norm per network).  CPU-only."""
import numpy as np
import pytest
import torch

from oracle import ppo_oracle as po
from tests import ppo_grad_reference as R
from tests.test_oracle_ppo import MIR_ACT, MIR_OBS

D, A = 37, 12
STDS = np.linspace(0.15, 0.4, A).astype(np.float32)
NO_CLIP = 1e9


def _obs_norm(rs):
    return rs.normal(size=D).astype(np.float32) * 0.3, (0.5 + rs.uniform(size=D)).astype(np.float32)


def _normalised(obs, mean, std, mo):
    """xn and xm in float32 with the oracle's (and lhw_ppo_normalize's) arithmetic: the same bits as the oracle's own inputs"""
    mean, std = torch.tensor(mean), torch.tensor(std)
    src, sign = mo
    mobs = obs[..., torch.as_tensor(src, dtype=torch.long)] * torch.as_tensor(sign)
    return (obs - mean) / std, (mobs - mean) / std


def _ff_case():
    rs = np.random.default_rng(11)
    H, B = 64, 200
    gen = torch.Generator().manual_seed(1)
    theta = {}
    for net, O in (("a", A), ("c", 1)):
        shapes = dict(w1=(H, D), b1=(H,), w2=(H, H), b2=(H,), w3=(O, H), b3=(O,))
        for n, s in shapes.items():
            theta[f"{net}_{n}"] = (torch.randn(*s, generator=gen) * (0.1 if n[0] == "b" else 1.0 / np.sqrt(s[-1]))).numpy()
    theta["stds"] = STDS
    mean, std = _obs_norm(rs)
    mo, ma = po.mirror_tables(MIR_OBS, [29, 30]), po.mirror_tables(MIR_ACT)
    obs = torch.tensor(rs.normal(size=(B, D)).astype(np.float32)) * torch.tensor(std) + torch.tensor(mean)
    xn, xm = _normalised(obs, mean, std, mo)
    act, old_logp, adv, ret = R.ff_inputs(theta, xn, [np.arange(B)], rs)
    smask = torch.tensor(rs.uniform(size=B) < 0.5)
    aidx = torch.tensor([0, 2, 5])
    target = torch.tensor(rs.normal(size=(int(smask.sum()), 3)).astype(np.float32))
    dense, mask = torch.zeros(B, A), torch.zeros(B, A, dtype=torch.uint8)
    rows = torch.nonzero(smask)[:, 0]
    dense[rows[:, None], aidx[None, :]] = target
    mask[rows[:, None], aidx[None, :]] = 1
    kw = dict(entropy_coeff=0.01, learn_std=True, mirror_act=ma, imitation=(0.5, dense, mask, int(mask.sum())))
    ref = lambda **k: R.ff_reference(theta, xn, xm, act, old_logp, adv, ret, **kw, **k)
    orc = po.OraclePPO([theta[f"a_{n}"] for n in R.FF_NET], [theta[f"c_{n}"] for n in R.FF_NET], STDS, mean, std, entropy_coeff=0.01,
                       max_grad_norm=NO_CLIP, learn_std=True, mirror_obs=mo, mirror_act=ma)
    res = orc.update(obs, act, ret[:, None], adv[:, None], old_logp[:, None], imit=(0.5, smask, aidx, target))
    grads = {f"a_{n}": p.grad.numpy() for n, p in zip(R.FF_NET, orc.actor)}
    grads.update({f"c_{n}": p.grad.numpy() for n, p in zip(R.FF_NET, orc.critic)})
    grads["stds"] = orc.stds.grad.numpy()
    stats = [res[0], res[2], res[4], res[3], res[6], res[5]]
    return ref, grads, stats, R.FF_MUTATIONS, dict(mirror=True, learn_std=True, imitation=True), adv.numpy()


def _rnn_case():
    rs = np.random.default_rng(12)
    H, T, B = 32, 12, 7
    gen = torch.Generator().manual_seed(2)
    theta = {}
    for net, O in (("a", A), ("c", 1)):
        shapes = dict(wih1=(4 * H, D), whh1=(4 * H, H), bih1=(4 * H,), bhh1=(4 * H,), wih2=(4 * H, H), whh2=(4 * H, H), bih2=(4 * H,),
                      bhh2=(4 * H,), wout=(O, H), bout=(O,))
        for n, s in shapes.items():
            theta[f"{net}_{n}"] = (torch.randn(*s, generator=gen) * (0.1 if n[0] == "b" else 1.0 / np.sqrt(s[-1]))).numpy()
    theta["stds"] = STDS
    mean, std = _obs_norm(rs)
    mo, ma = po.mirror_tables(MIR_OBS, [29, 30]), po.mirror_tables(MIR_ACT)
    obs = torch.tensor(rs.normal(size=(T, B, D)).astype(np.float32)) * torch.tensor(std) + torch.tensor(mean)
    reset = torch.tensor(rs.uniform(size=(T, B)) < 0.15)
    reset[0] = True
    reset[1:, 0] = False          # one column without an episode start inside it
    reset[T - 1, 1] = True        # one that starts an episode at its last step
    xn, xm = _normalised(obs, mean, std, mo)
    act, old_logp, adv, ret = R.rnn_inputs(theta, xn, reset, [np.arange(B)], rs)
    ref = lambda **k: R.rnn_reference(theta, xn, xm, reset, act, old_logp, adv, ret, mirror_act=ma, **k)
    orc = po.OracleRecurrentPPO([theta[f"a_{n}"] for n in R.RNN_NET], [theta[f"c_{n}"] for n in R.RNN_NET], STDS, mean, std,
                                max_grad_norm=NO_CLIP, mirror_obs=mo, mirror_act=ma)
    a_loss, c_loss, m_loss = orc.update(obs, reset, act, ret[..., None], adv[..., None], old_logp[..., None])
    grads = {f"a_{n}": p.grad.numpy() for n, p in zip(R.RNN_NET, orc.actor)}
    grads.update({f"c_{n}": p.grad.numpy() for n, p in zip(R.RNN_NET, orc.critic)})
    grads["stds"] = np.zeros(A, np.float32)
    stats = [a_loss, c_loss, m_loss, None, None, 0.0]
    return ref, grads, stats, R.RNN_MUTATIONS, dict(mirror=True, learn_std=False), adv.numpy()


@pytest.fixture(scope="module", params=["feed-forward", "recurrent"])
def case(request):
    ref, grads, stats, mutations, active, adv = (_ff_case if request.param == "feed-forward" else _rnn_case)()
    ref64 = ref(want_rows=True)
    return dict(kind=request.param, ref=ref, ref64=ref64, ref32=ref(dtype=torch.float32, want_rows=True), ratio=ref64[2]["ratio"], grads=grads, stats=stats,
                mutations=mutations, active=active, adv=adv)


def test_inputs_populate_every_branch_of_the_head(case):
    counts = R.class_counts(case["ratio"], case["adv"])
    print(case["kind"], counts)
    assert min(counts.values()) >= 2, counts
    assert 0.2 < case["ref64"][0][4] < 0.8      # clip fraction: rows on both sides


def test_reference_agrees_with_the_oracle(case):
    s64, g64 = case["ref64"][:2]
    stats = list(case["stats"])
    for i in (3, 4):      # the recurrent oracle reports no approx_kl / clip fraction: nothing to compare them with
        if stats[i] is None:
            stats[i] = s64[i]
    worst, name, worst_y, name_y, fails = R.compare(case["grads"], stats, case["ref64"], case["ref32"])
    print(f"{case['kind']}: oracle vs float64 reference: worst error / bar {worst:.3g} ({name}), worst error / own y {worst_y:.3g} ({name_y})")
    assert not fails, fails
    assert set(case["grads"]) == set(g64)


def test_float32_yardstick_is_float32_roundoff(case):
    """the yardstick itself: far above float64's roundoff and below 1e-5 on every tensor, so a bar of MARGIN x y pins five digits or more"""
    y = R.yardstick(case["ref32"][1], case["ref64"][1])
    print(case["kind"], {n: f"{v:.2g}" for n, v in y.items()})
    assert all(1e-9 < v < 1e-5 for v in y.values()), y


def test_every_mutation_moves_the_reference_gradient(case):
    for m in case["mutations"]:
        # (the recurrent oracle has no learnable stds: the entropy mutation is checked on the same case with them switched on)
        extra = {} if R.mutation_is_active(m, **case["active"]) else dict(learn_std=True, entropy_coeff=0.01)
        assert not extra or m == "entropy_x2"
        g64 = case["ref"](**extra)[1] if extra else case["ref64"][1]      # this mutation's own baseline
        _, gm = case["ref"](mutation=m, **extra)
        moved = {}
        for net in ("actor", "critic"):
            names = [n for n in g64 if R._network(n) == net]
            top = max(float(np.abs(g64[n]).max()) for n in names)
            moved[net] = max(float(np.abs(gm[n] - g64[n]).max()) for n in names) / top
        print(f"{case['kind']} {m}: moved {moved}")
        assert max(moved.values()) >= 1e-3, (m, moved)


def _reordered_float32(theta, xn, xm, act, old_logp, adv, ret, rs, **kw):
    """The feed-forward reference in float32 with the hidden units and the minibatch rows permuted -- the same function summed in another order,
    as a kernel sums it -- with the gradients put back in the original order."""
    H, B = theta["a_b1"].shape[0], xn.shape[0]
    p1, p2, pr = rs.permutation(H), rs.permutation(H), rs.permutation(B)
    t2 = dict(theta)
    for net in "ac":
        t2[f"{net}_w1"], t2[f"{net}_b1"] = theta[f"{net}_w1"][p1], theta[f"{net}_b1"][p1]
        t2[f"{net}_w2"], t2[f"{net}_b2"] = theta[f"{net}_w2"][p2][:, p1], theta[f"{net}_b2"][p2]
        t2[f"{net}_w3"] = theta[f"{net}_w3"][:, p2]
    if kw.get("imitation") is not None:
        coeff, target, mask, count = kw["imitation"]
        kw = dict(kw, imitation=(coeff, target[pr], mask[pr], count))
    s, g2 = R.ff_reference(t2, xn[pr], None if xm is None else xm[pr], act[pr], old_logp[pr], adv[pr], ret[pr], dtype=torch.float32, **kw)
    g = dict(g2)
    i1, i2 = np.argsort(p1), np.argsort(p2)
    for net in "ac":
        g[f"{net}_w1"], g[f"{net}_b1"] = g2[f"{net}_w1"][i1], g2[f"{net}_b1"][i1]
        g[f"{net}_w2"], g[f"{net}_b2"] = g2[f"{net}_w2"][i2][:, i1], g2[f"{net}_b2"][i2]
        g[f"{net}_w3"] = g2[f"{net}_w3"][:, i2]
    return s, g


@pytest.mark.parametrize("B,mirror", [(33, False), (33, True), (200, False), (256, False), (256, True)])
def test_another_summation_order_stays_within_the_bars(B, mirror):
    """The bars must pass what is only float32 roundoff: the reference in float32 with the hidden units and the rows in another order lies within
    them, over six draws of weights and inputs per shape, tensors and loss scalars alike.  (With |s32 - s64| alone as a scalar's yardstick this
    fails: one evaluation's error of a cancelling sum is one draw, and comes out far below its scale often enough.)"""
    H = 256
    mo, ma = po.mirror_tables(MIR_OBS, [29, 30]), po.mirror_tables(MIR_ACT)
    worst_seen = 0.0
    for seed in range(6):
        rs = np.random.default_rng(100 * seed + B)
        theta = {}
        for net, O in (("a", A), ("c", 1)):
            for n, s in dict(w1=(H, D), b1=(H,), w2=(H, H), b2=(H,), w3=(O, H), b3=(O,)).items():
                w = rs.normal(size=s)
                theta[f"{net}_{n}"] = (w / np.sqrt((w ** 2).sum(1, keepdims=True)) if len(s) == 2 else 0.1 * w).astype(np.float32)
        theta["stds"] = STDS
        xn = rs.normal(size=(B, D)).astype(np.float32)
        xm = (xn[:, mo[0]] * mo[1]).astype(np.float32) if mirror else None
        act, old_logp, adv, ret = (t.numpy() for t in R.ff_inputs(theta, xn, [np.arange(B)], rs))
        kw = dict(learn_std=True, entropy_coeff=0.01, mirror_act=ma if mirror else None)
        args = (theta, xn, xm, act, old_logp, adv, ret)
        ref64, ref32 = R.ff_reference(*args, want_rows=True, **kw), R.ff_reference(*args, dtype=torch.float32, want_rows=True, **kw)
        s, g = _reordered_float32(*args, rs, **kw)
        worst, name, worst_y, name_y, fails = R.compare(g, s, ref64, ref32)
        print(f"B {B} mirror {mirror} seed {seed}: worst error / y {R.MARGIN * worst:.3g} ({name}); over each tensor's own y {worst_y:.3g} ({name_y})")
        assert not fails, fails
        worst_seen = max(worst_seen, R.MARGIN * worst)
    assert worst_seen < R.MARGIN
