"""The optimiser step of the update path: clip_grad_norm_ + Adam (sumsq2_kernel / adam2_kernel through lhw_ppo_apply / lhw_rnn_apply)
against torch's own clip_grad_norm_ and torch.optim.Adam in float64; the graph-replayed step (lhw_ppo_step) with a changing grad_scale;
and the padding lanes of the flat parameter vector through real updates."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LR, EPS, MAX_NORM = 1e-3, 1e-5, 0.5
# the kernels hold the hyper-parameters as float32 (0.999f is 0.99900001287: 1 - beta2 differs from 1e-3 by 1.3e-5 relative);
# the reference runs on exactly those values, so that what is compared is the arithmetic
F32 = lambda x: float(np.float32(x))
BETAS = (F32(0.9), F32(0.999))
# Bars, per element and step, in units of float32's unit roundoff u = 2^-24 = 6e-8 (worst-case bounds, not fits):
# - clip coefficient: the squared norm is a float32 sum of n <= 2e5 positive terms, at most 3 per lane, a 6-level wave tree, a 2-level
#   block tree and 128 block partials added in sequence: <= ~140 roundings, relative error <= 140 u = 8.3e-6; sqrt, + 1e-6 and the
#   division add 3 u.  => coefficient (and so the clipped gradient) relative error <= 9e-6.
# - adam_m: each step rounds g * grad_scale * coef (2 u, grad_scale a power of two is exact) and the two products and the sum of the
#   moving average (3 u); errors decay by beta1 per step.  Measured against m_abs, the same average of |g|: <= 9e-6 + 5 u / (1 - beta1)
#   = 1.2e-5.  BAR_M = 2e-5.
# - adam_v: the squared coefficient doubles its error (1.8e-5); g * g and the average add 4 u per step and decay only by beta2, so
#   over 44 steps <= 176 u = 1.1e-5.  Relative to v (all terms positive): 2.9e-5.  BAR_V = 5e-5.
# - the update u = lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps): BAR_M + BAR_V / 2 + ~8 u (powf, sqrt, divisions) relative to u_abs (u
#   with m_abs), BAR_U = 5e-5; plus the rounding of theta when it is stored: 1 ulp of |theta| (float32 spacing), absolute.
BAR_M, BAR_V, BAR_U = 2e-5, 5e-5, 5e-5
SCALES = [1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1, 1.0, 1e1, 1e2]
N_STEPS = 44
ZERO_STEP = 24          # (1-based, as Adam counts)


def _schedule():
    """(actor scale, critic scale, grad_scale) per step: both groups' scales sweep 1e-7 .. 1e2 independently (so that either group is
    clipped while the other is not), grad_scale cycles through 1, 0.5, 0.125 (every combination within 30 steps); one all-zero step."""
    out = []
    for t in range(N_STEPS):
        gs = (1.0, 0.5, 0.125)[t % 3]
        out.append((0.0, 0.0, gs) if t + 1 == ZERO_STEP else (SCALES[t % 10], SCALES[(3 * t + 5) % 10], gs))
    return out


def _pad4(n):
    return (n + 3) // 4 * 4


def _layout(k):
    """(off_std, off_critic, groups): the two parameter groups exactly as the kernels clip them -- actor [0, na) with na = off_std
    (+ act_dim if the stds are parameters), critic [off_critic, n_params)."""
    from learninghumanoidwalking_amd.ppo_kernels import PpoKernels
    off_std, off_critic = (k.offsets[6], k.offsets[7]) if isinstance(k, PpoKernels) else (k.offsets[8], k.offsets[9])
    assert off_critic == off_std + _pad4(k.act_dim)
    na = off_std + (k.act_dim if k.learn_std else 0)
    return off_std, off_critic, [(0, na), (off_critic, k.n_params)]


class _Reference:
    """float64 copies of the two groups stepped by torch.nn.utils.clip_grad_norm_ + torch.optim.Adam.  ``mutation`` (negative
    controls): "coef_x1.01" multiplies a clipped gradient by another 1.01; "norm_without_grad_scale" takes the clip coefficient from the
    unscaled gradient; "bias_correction_late" gives Adam the step count of the previous step (from step 2 on)."""

    def __init__(self, groups0, mutation=None):
        self.p = [torch.nn.Parameter(g.clone()) for g in groups0]
        self.opt = torch.optim.Adam([{"params": [p]} for p in self.p], lr=F32(LR), betas=BETAS, eps=F32(EPS), foreach=False)
        self.mutation, self.t = mutation, 0

    def step(self, grads, gs):
        self.t += 1
        clipped = []
        for p, g in zip(self.p, grads):
            if self.mutation == "norm_without_grad_scale":
                p.grad = g.clone()
                norm = torch.nn.utils.clip_grad_norm_([p], MAX_NORM)
                p.grad.mul_(gs)
            else:
                p.grad = g * gs
                norm = torch.nn.utils.clip_grad_norm_([p], MAX_NORM)
                if self.mutation == "coef_x1.01" and MAX_NORM / (float(norm) + 1e-6) < 1:
                    p.grad.mul_(1.01)
            clipped.append(MAX_NORM / (float(norm) + 1e-6) < 1)
        if self.mutation == "bias_correction_late" and self.t >= 2:
            for p in self.p:
                self.opt.state[p]["step"].fill_(self.t - 2)     # Adam adds one before it corrects: step t uses t - 1
        gabs = [p.grad.abs() for p in self.p]
        self.opt.step()
        return clipped, gabs

    def state(self):
        return [(p.detach().clone(), self.opt.state[p]["exp_avg"].clone(), self.opt.state[p]["exp_avg_sq"].clone()) for p in self.p]


def _handle(kind, hidden, learn_std, D, A):
    if kind == "ppo":
        from learninghumanoidwalking_amd.ppo_kernels import PpoKernels
        return PpoKernels(D, A, hidden=hidden, max_rows=64, learn_std=learn_std, lr=LR, eps=EPS, max_grad_norm=MAX_NORM)
    from learninghumanoidwalking_amd.rnn_kernels import RnnKernels
    return RnnKernels(D, A, hidden=hidden, seq_len=24, seq_cols=6, rollout_rows=10, learn_std=learn_std, lr=LR, eps=EPS,
                      max_grad_norm=MAX_NORM)


CASES = [("ppo", h, ls, d, a) for h in (64, 256) for ls in (False, True) for (d, a) in ((37, 12), (35, 10))] + \
        [("rnn", 32, False, 37, 12), ("rnn", 64, True, 37, 12)]


@pytest.mark.parametrize("kind,hidden,learn_std,D,A", CASES, ids=[f"{c[0]}-h{c[1]}-{'std' if c[2] else 'fixedstd'}-{c[3]}x{c[4]}" for c in CASES])
def test_clip_and_adam_match_torch_in_float64(kind, hidden, learn_std, D, A):
    k = _handle(kind, hidden, learn_std, D, A)
    off_std, off_critic, groups = _layout(k)
    n = k.n_params
    rs = np.random.default_rng(hidden * 1000 + D * 10 + learn_std)
    theta0 = rs.uniform(-1e-2, 1e-2, size=n).astype(np.float32)
    k.theta.copy_(torch.from_numpy(theta0))
    g64 = lambda x: torch.from_numpy(np.asarray(x, dtype=np.float64))
    refs = {m: _Reference([g64(theta0[a:b]) for a, b in groups], m)
            for m in (None, "coef_x1.01", "norm_without_grad_scale", "bias_correction_late")}
    m_abs = [torch.zeros(b - a, dtype=torch.float64) for a, b in groups]
    worst = {m: 0.0 for m in refs}
    seen = dict(both=0, neither=0, actor_only=0, critic_only=0, below_eps=0, gs_clipped=set())
    theta_prev = theta0.astype(np.float64)
    prev = {m: [theta_prev[a:b].copy() for a, b in groups] for m in refs}
    for t, (sa, sc, gs) in enumerate(_schedule(), 1):
        g = np.zeros(n, dtype=np.float32)
        for (a, b), s in zip(groups, (sa, sc)):
            # log-uniform magnitudes over four decades, random signs: after clipping, most entries sit far below the largest,
            # many of them below Adam's eps, where the update is linear in the gradient (a wrong coefficient shows 1:1)
            g[a:b] = s * rs.choice([-1.0, 1.0], size=b - a) * 10.0 ** rs.uniform(-4, 0, size=b - a)
        if not learn_std:
            g[off_std:off_critic] = 1e3         # the stds are not parameters: the kernels must neither clip with nor apply these
        k.grad.copy_(torch.from_numpy(g))
        k.apply(grad_scale=gs)
        grads = [g64(g[a:b]) for a, b in groups]
        ref_sq = [float(((gs * x) ** 2).sum()) for x in grads]
        clipped = gabs = None
        for m, r in refs.items():
            c, ga = r.step(grads, gs)
            if m is None:
                clipped, gabs = c, ga
        sq = k.debug_grad_sqnorms()
        th, mm, vv = (x.cpu().numpy().astype(np.float64) for x in (k.theta, k.adam_m, k.adam_v))
        assert not k.grad.any(), f"step {t}: the gradient is not zeroed"
        assert np.isfinite(th).all() and np.isfinite(mm).all() and np.isfinite(vv).all(), f"step {t}: non-finite state"
        # the squared norms the kernel clipped with: a float32 sum of float32 squares (bound above: 140 u), vs float64
        for grp in range(2):
            assert abs(sq[grp] - ref_sq[grp]) <= 1e-5 * ref_sq[grp], (t, grp, sq[grp], ref_sq[grp])
        if t == ZERO_STEP:
            assert sq == (0.0, 0.0)
        # the stds (not parameters) and the gap between the groups keep their values; their Adam state stays zero
        gap = slice(groups[0][1], off_critic)
        assert np.array_equal(th[gap], theta0[gap].astype(np.float64)) and not mm[gap].any() and not vv[gap].any(), t
        # tolerances from the true reference
        st = refs[None].state()
        bc1, bc2 = 1 - BETAS[0] ** t, 1 - BETAS[1] ** t
        tol = []
        for grp, (a, b) in enumerate(groups):
            m_abs[grp].mul_(BETAS[0]).add_((1 - BETAS[0]) * gabs[grp])
            v_ref = st[grp][2].numpy()
            u_abs = F32(LR) / bc1 * m_abs[grp].numpy() / (np.sqrt(v_ref / bc2) + F32(EPS))
            spacing = np.spacing(np.maximum(np.abs(th[a:b]), np.abs(theta_prev[a:b])).astype(np.float32)).astype(np.float64)
            tol.append((BAR_U * u_abs + spacing, BAR_M * m_abs[grp].numpy() + 1e-45, BAR_V * v_ref + 1e-45))
        # this step's movement of theta (not the accumulated one: float32 storage rounding does not pile up), adam_m and adam_v
        for m, r in refs.items():
            now = r.state()
            for grp, ((a, b), (p, em, ev)) in enumerate(zip(groups, now)):
                d_kernel, d_ref = th[a:b] - theta_prev[a:b], p.numpy() - prev[m][grp]
                e = max(float((np.abs(d_kernel - d_ref) / tol[grp][0]).max()), float((np.abs(mm[a:b] - em.numpy()) / tol[grp][1]).max()),
                        float((np.abs(vv[a:b] - ev.numpy()) / tol[grp][2]).max()))
                worst[m] = max(worst[m], e)
            prev[m] = [p.numpy() for p, _, _ in now]
        assert worst[None] <= 1.0, f"step {t} (scales {sa:g} / {sc:g}, grad_scale {gs}): error {worst[None]:.3g} x the bar"
        theta_prev = th
        ca, cc = clipped
        seen["both" if ca and cc else "neither" if not (ca or cc) else "actor_only" if ca else "critic_only"] += 1
        if ca and cc:
            seen["gs_clipped"].add(gs)
        if t != ZERO_STEP and max(float(x.max()) for x in gabs) < EPS:
            seen["below_eps"] += 1
    # the schedule exercised what it is meant to
    assert min(seen["both"], seen["neither"], seen["actor_only"], seen["critic_only"], seen["below_eps"]) >= 2, seen
    assert seen["gs_clipped"] == {1.0, 0.5, 0.125}, seen
    # negative controls: each mutated reference is rejected by at least 10x the bar, or the bar is too loose to see it
    for m in ("coef_x1.01", "norm_without_grad_scale", "bias_correction_late"):
        assert worst[m] >= 10.0, f"negative control {m}: only {worst[m]:.3g} x the bar"
    print(f"{kind} h{hidden} learn_std={learn_std} {D}x{A}: worst error {worst[None]:.3g} x bar; negative controls " +
          ", ".join(f"{m} {worst[m]:.3g}" for m in worst if m))


# D = 35, A = 10: every kind of padding exists (W1 columns 35, the actor read-out rows 10 and 11, two std slots)
PAD_D, PAD_A = 35, 10
PAD_MIR_OBS = [v for i in range(17) for v in (2 * i + 1, -(2 * i) if i else -0.1)] + [34]
PAD_MIR_ACT = [5, -6, 7, 8, -9, 0.1, -1, 2, 3, -4]


def _ppo_batch(k, rs, R, idx_count, B):
    """Observations, rollout actions / log-probs from the handle's own policy, random advantages / returns, and idx_count random
    minibatches of B rows."""
    obs = torch.tensor(rs.normal(size=(R, k.obs_dim)).astype(np.float32)).cuda()
    act = torch.empty(R, k.act_dim, device="cuda")
    logp = torch.empty(R, device="cuda")
    for r0 in range(0, R, k.max_rows):      # the forward workspace holds max_rows rows
        _, act[r0:r0 + k.max_rows], logp[r0:r0 + k.max_rows], _ = k.forward(obs[r0:r0 + k.max_rows], seed=5, env_id_base=r0)
    adv = torch.tensor(rs.normal(size=R).astype(np.float32)).cuda()
    ret = torch.tensor(rs.normal(size=R).astype(np.float32)).cuda()
    xn, xm = k.normalize(obs)
    idx = [torch.tensor(rs.permutation(R)[:B].astype(np.int32)).cuda() for _ in range(idx_count)]
    return xn, xm, act, logp, adv, ret, idx


def test_graph_step_follows_a_changing_grad_scale(monkeypatch):
    """lhw_ppo_step with grad_scale 1, 1, 0.5, 0.5, 0.125, 1 is bitwise lhw_ppo_grad + lhw_ppo_apply with the same scales.  Clipping is
    active (max_grad_norm 1e-3), so a graph replayed with the scale it was first captured with clips with the wrong norm."""
    from learninghumanoidwalking_amd.ppo_kernels import PpoKernels, reference_init
    monkeypatch.delenv("LHW_PPO_GRAPH", raising=False)
    D, A, H, B = PAD_D, PAD_A, 64, 256
    w = reference_init(D, A, H, 0.223, generator_seed=4)
    ks = [PpoKernels(D, A, hidden=H, max_rows=B, lr=1e-3, max_grad_norm=1e-3) for _ in range(2)]
    for k in ks:
        k.set_tensors(w)
    rs = np.random.default_rng(2)
    stream = torch.cuda.Stream()        # not the legacy default stream: that one cannot be captured (the library goes eager)
    with torch.cuda.stream(stream):
        xn, xm, act, logp, adv, ret, idx = _ppo_batch(ks[0], rs, 1024, 6, B)
        graph, eager = ks
        for t, gs in enumerate([1.0, 1.0, 0.5, 0.5, 0.125, 1.0]):
            graph.step_minibatch(xn, None, act, logp, adv, ret, idx[t], grad_scale=gs)
            eager.grad_minibatch(xn, None, act, logp, adv, ret, idx[t])
            eager.apply(grad_scale=gs)
            sq_g, sq_e = graph.debug_grad_sqnorms(), eager.debug_grad_sqnorms()
            assert min(sq_e) > 1e-6, f"step {t}: clipping is not active ({sq_e})"
            assert sq_g == sq_e, f"step {t} (grad_scale {gs}): squared norms {sq_g} (graph) vs {sq_e} (two calls)"
            for name in ("theta", "adam_m", "adam_v"):
                assert torch.equal(getattr(graph, name), getattr(eager, name)), f"step {t} (grad_scale {gs}): {name} differs"
            assert torch.equal(graph.stats[:5], eager.stats[:5]), t
            assert not graph.grad.any() and not eager.grad.any()


def _padding_mask(k):
    """True at every padding entry of the flat PPO vector (lhw_ppo_layout offsets): W1 columns obs_dim..Dp of both networks, the actor
    read-out rows act_dim..Op, the critic read-out rows 1..3 (weights and biases), std slots act_dim..pad4(act_dim)."""
    H, D, A, Dp, Op = k.hidden, k.obs_dim, k.act_dim, k.Dp, k.Op
    off = dict(zip(k.TENSORS, k.offsets))
    m = torch.zeros(k.n_params, dtype=torch.bool)
    for net, rows, op in (("a", A, Op), ("c", 1, 4)):
        m[off[f"{net}_w1"]:off[f"{net}_w1"] + H * Dp].view(H, Dp)[:, D:] = True
        m[off[f"{net}_w3"]:off[f"{net}_w3"] + op * H].view(op, H)[rows:] = True
        m[off[f"{net}_b3"] + rows:off[f"{net}_b3"] + op] = True
    m[off["stds"] + A:off["stds"] + _pad4(A)] = True
    assert int(m.sum()) == 2 * H * (Dp - D) + (Op - A) * (H + 1) + 3 * (H + 1) + (_pad4(A) - A)
    return m.cuda()


@pytest.mark.parametrize("path", ["two_calls", "graph"])
@pytest.mark.parametrize("learn_std", [False, True])
@pytest.mark.parametrize("hidden", [64, 256])
def test_padding_stays_exactly_zero_through_real_updates(hidden, learn_std, path):
    """The clip norm sums the flat ranges, padding included: it equals torch's per-tensor norm only if every padding gradient is 0.
    Real minibatch updates (mirror loss on, entropy bonus on the stds when they are parameters): the gradient after lhw_ppo_grad and
    theta / adam_m / adam_v after the optimiser step are exactly 0 at every padding entry."""
    from learninghumanoidwalking_amd.ppo_kernels import PpoKernels, reference_init
    from oracle import ppo_oracle as po
    D, A, B = PAD_D, PAD_A, 512
    k = PpoKernels(D, A, hidden=hidden, max_rows=B, learn_std=learn_std, entropy_coeff=0.01 if learn_std else 0.0, lr=1e-3,
                   mirror_obs=po.mirror_tables(PAD_MIR_OBS), mirror_act=po.mirror_tables(PAD_MIR_ACT))
    k.set_tensors(reference_init(D, A, hidden, 0.223, generator_seed=hidden + learn_std))
    pad = _padding_mask(k)
    stds = slice(k.offsets[6], k.offsets[7])
    rs = np.random.default_rng(hidden + 2 * learn_std)
    k.set_obs_norm(rs.normal(size=D).astype(np.float32) * 0.1, (0.5 + rs.uniform(size=D)).astype(np.float32))
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        xn, xm, act, logp, adv, ret, idx = _ppo_batch(k, rs, 2048, 4, B)
        assert not xn[:, D:].any() and not xm[:, D:].any()
        theta0 = k.theta.clone()
        for t in range(4):
            if path == "graph":
                k.step_minibatch(xn, xm, act, logp, adv, ret, idx[t])
            else:
                k.grad_minibatch(xn, xm, act, logp, adv, ret, idx[t])
                stream.synchronize()
                assert k.grad.abs().sum() > 0
                bad = int(k.grad[pad].count_nonzero())
                assert bad == 0, f"update {t}: {bad} padding entries of the gradient are non-zero"
                if not learn_std:
                    assert not k.grad[stds].any()
                k.apply()
            stream.synchronize()
            for name in ("theta", "adam_m", "adam_v"):
                bad = int(getattr(k, name)[pad].count_nonzero())
                assert bad == 0, f"update {t}: {bad} padding entries of {name} are non-zero"
            assert not k.grad.any()
        assert not torch.equal(k.theta, theta0)
        if not learn_std:
            assert torch.equal(k.theta[stds], theta0[stds]) and not k.adam_m[stds].any()


@pytest.mark.parametrize("recurrent", [False, True])
def test_optimizer_views_are_the_slices_of_the_adam_moments(recurrent, tmp_path):
    """PPO.actor_optimizer / critic_optimizer (the reference's two torch.optim.Adam, rl/algos/ppo.py:128-129) as views of the flat Adam
    moments, feed-forward and LSTM: after one iteration every entry's exp_avg / exp_avg_sq is that tensor's slice of adam_m / adam_v, the
    two optimisers split the tensors between them, and (with every position of adam_m numbered) the entries have the shapes of the
    reference's parameters and read disjoint positions."""
    from types import SimpleNamespace
    from learninghumanoidwalking_amd.envs import ENVIRONMENTS
    from learninghumanoidwalking_amd.ppo import PPO
    from learninghumanoidwalking_amd.ppo_kernels import reference_init
    from learninghumanoidwalking_amd.rnn_kernels import reference_init_lstm
    args = SimpleNamespace(gamma=0.99, lam=0.95, lr=3e-4, eps=1e-5, entropy_coeff=0.0, clip=0.2, minibatch_size=16 if recurrent else 256,
                           epochs=1, max_traj_len=12, num_procs=32, num_envs=32, max_grad_norm=0.5, mirror_coeff=0.4, eval_freq=10**9,
                           recurrent=recurrent, imitate=None, learn_std=False, std_dev=0.223, no_mirror=False, continued=None,
                           logdir=str(tmp_path), device_index=0, lstm_hidden=64)
    algo = PPO(ENVIRONMENTS["jvrc_walk"], args, seed=5)
    algo.iterate(0)
    k = algo.kernels
    assert k.adam_step > 0
    sa, sc = algo.actor_optimizer.state_dict(), algo.critic_optimizer.state_dict()
    names = list(sa["state"]) + list(sc["state"])
    assert sorted(names) == sorted(k.get_tensors()) and len(set(names)) == len(names)
    assert all(n.startswith("a_") or n == "stds" for n in sa["state"]) and all(n.startswith("c_") for n in sc["state"])
    m, v = k.get_tensors(k.adam_m), k.get_tensors(k.adam_v)
    for st in (sa["state"], sc["state"]):
        for n, e in st.items():
            assert e["step"] == k.adam_step
            assert torch.equal(e["exp_avg"], m[n]) and torch.equal(e["exp_avg_sq"], v[n]), n
    assert any(e["exp_avg"].any() for e in sa["state"].values()) and any(e["exp_avg"].any() for e in sc["state"].values())
    # number every position of adam_m: the entries then name the positions they read
    assert k.n_params < 2 ** 24
    k.adam_m.copy_(torch.arange(k.n_params, dtype=torch.float32, device=k.adam_m.device))
    ref = (reference_init_lstm(k.obs_dim, k.act_dim, k.hidden) if recurrent else reference_init(k.obs_dim, k.act_dim, k.hidden))
    pos = []
    for opt in (algo.actor_optimizer, algo.critic_optimizer):
        for n, e in opt.state_dict()["state"].items():
            assert e["exp_avg"].shape == ref[n].shape, n
            pos.append(e["exp_avg"].reshape(-1).long())
    pos = torch.cat(pos)
    assert pos.numel() == sum(t.numel() for t in ref.values()) == pos.unique().numel()
