"""The PPO minibatch loss in plain torch with autograd: the reference of what lhw_ppo_grad / lhw_rnn_grad leave in ``grad`` and ``stats[:6]``.
TEST INFRASTRUCTURE ONLY (a helper module, not a conftest).

Written from the loss definition (reference rl/algos/ppo.py:299-406 as oracle/ppo_oracle.py:111-151 and :205-229 state it), on the NORMALISED
inputs the kernels are given: ``xn`` and the mirrored ``xm`` (lhw_ppo_normalize builds both).  The float32 weights, observations, actions, old
log-probabilities, advantages and returns are taken exactly and widened to ``dtype``; float64 is the reference, the SAME function in float32 on the
CPU is the yardstick of float32 roundoff (``yardstick`` / ``bars`` below).

    loss = actor + mirror_coeff * mirror + imit_coeff * imitation + entropy_coeff * entropy_penalty + critic
    actor   = -mean_B min(ratio * adv, clamp(ratio, 1 - clip, 1 + clip) * adv),  ratio = exp(logp - old_logp)
    critic  = mean_B (ret - v)^2
    mirror  = mean_{B A} (mu - sign_a * mu_twin[src_a])^2
    imitation = sum over the selected (row, action) entries of (mu - target)^2 / n_selected
    entropy_penalty = -mean_A (0.5 + 0.5 log 2 pi + log std_a)        (stds are parameters only with learn_std)

Returned: the six loss scalars in ``stats`` order (actor, critic, mirror, approx_kl, clip_fraction, imitation) as a float64 numpy vector, and
the gradient of every named tensor (the stds' is zero where they are not parameters) as {name: float64 numpy array}.

``mutation`` (negative controls, each a deliberate mistake in the GRADIENT; the scalars stay those of the true loss where the mistake is a factor):
"critic_half" (MSE without the 2), "ppo_x1.01" (PPO term against an unchanged mirror term), "mirror_mean_over_B", "no_min" (clipped rows let
through), "entropy_x2", "imit_denominator_Bk", "twin_detached", and for the recurrent form "resets_ignored", "cell_state_cut" (no gradient
through the cell state across one step, T // 2)."""
from __future__ import annotations

import math

import numpy as np
import torch

MARGIN = 8.0
SCALARS = ("actor_loss", "critic_loss", "mirror_loss", "approx_kl", "clip_fraction", "imitation_loss")
FF_MUTATIONS = ("critic_half", "ppo_x1.01", "mirror_mean_over_B", "no_min", "entropy_x2", "imit_denominator_Bk", "twin_detached")
RNN_MUTATIONS = ("critic_half", "ppo_x1.01", "mirror_mean_over_B", "no_min", "entropy_x2", "twin_detached", "resets_ignored", "cell_state_cut")
FF_NET = ("w1", "b1", "w2", "b2", "w3", "b3")
RNN_NET = ("wih1", "whh1", "bih1", "bhh1", "wih2", "whh2", "bih2", "bhh2", "wout", "bout")


def mutation_is_active(mutation, *, mirror, learn_std, imitation=False):
    """Whether the term a mutation touches is part of the case's loss."""
    if mutation in ("mirror_mean_over_B", "twin_detached"):
        return mirror
    if mutation == "entropy_x2":
        return learn_std
    if mutation == "imit_denominator_Bk":
        return imitation
    return True


def _mlp(x, p):
    h = torch.relu(x @ p["w1"].T + p["b1"])
    h = torch.relu(h @ p["w2"].T + p["b2"])
    return h @ p["w3"].T + p["b3"]


def _cell(x, h, c, wih, whh, bih, bhh):
    """One LSTM cell from its definition, gate by gate (rows [0, H) input, [H, 2H) forget, [2H, 3H) candidate, [3H, 4H) output gate):
    c' = sigma(f) c + sigma(i) tanh(g), h' = sigma(o) tanh(c')."""
    H = h.shape[-1]
    pre = [torch.nn.functional.linear(x, wih[k * H:(k + 1) * H], bih[k * H:(k + 1) * H]) +
           torch.nn.functional.linear(h, whh[k * H:(k + 1) * H], bhh[k * H:(k + 1) * H]) for k in range(4)]
    sig = lambda v: 1.0 / (1.0 + torch.exp(-v))
    c = sig(pre[1]) * c + sig(pre[0]) * torch.tanh(pre[2])
    return sig(pre[3]) * torch.tanh(c), c


def _lstm(x, reset, p, cut_at=None):
    """x [T, B, D], reset [T, B] bool (an episode starts at step t of the column: the state is zero there) -> read-out [T, B, O]"""
    T, B, _ = x.shape
    H = p["whh1"].shape[1]
    zero = torch.zeros(B, H, dtype=x.dtype)
    h1 = c1 = h2 = c2 = zero
    ys = []
    for t in range(T):
        start = reset[t].unsqueeze(-1)
        h1, c1, h2, c2 = (torch.where(start, zero, s) for s in (h1, c1, h2, c2))
        if cut_at is not None and t == cut_at:
            c1, c2 = c1.detach(), c2.detach()
        h1, c1 = _cell(x[t], h1, c1, p["wih1"], p["whh1"], p["bih1"], p["bhh1"])
        h2, c2 = _cell(h1, h2, c2, p["wih2"], p["whh2"], p["bih2"], p["bhh2"])
        ys.append(h2 @ p["wout"].T + p["bout"])
    return torch.stack(ys)


def _loss_and_grad(theta, names, net, act, old_logp, adv, ret, *, clip, mirror_coeff, entropy_coeff, learn_std, mirror_act, imitation,
                   dtype, mutation):
    """``net(params of one network, twin: bool)`` -> read-out with the sample axes flattened to [M, O]; act [M, A]; old_logp / adv / ret [M]."""
    w = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)
    P = {n: w(theta[n]).clone().requires_grad_(n != "stds" or learn_std) for n in list(names) + ["stds"]}
    pa = {n[2:]: P[n] for n in names if n.startswith("a_")}
    pc = {n[2:]: P[n] for n in names if n.startswith("c_")}
    act, old_logp, adv, ret = w(act), w(old_logp).reshape(-1), w(adv).reshape(-1), w(ret).reshape(-1)
    M, A = act.shape
    stds = P["stds"]
    mu = net(pa, False)
    z = (act - mu) / stds
    logp = (-0.5 * z * z - torch.log(stds) - 0.5 * math.log(2.0 * math.pi)).sum(-1)
    logr = logp - old_logp
    ratio = torch.exp(logr)
    cpi = ratio * adv
    clipped = ratio.clamp(1.0 - clip, 1.0 + clip) * adv
    actor = -(cpi if mutation == "no_min" else torch.minimum(cpi, clipped)).mean()
    zero = torch.zeros((), dtype=dtype)
    rows = {0: -torch.minimum(cpi, clipped), 1: (ret - net(pc, False)[:, 0]).pow(2), 2: zero.expand(M), 3: (ratio - 1.0) - logr, 5: zero.expand(M)}
    actor_true, critic = rows[0].mean(), rows[1].mean()
    mirror = mirror_g = zero
    if mirror_act is not None:
        src, sign = mirror_act
        twin = net(pa, True)
        if mutation == "twin_detached":
            twin = twin.detach()
        twin = twin[:, torch.as_tensor(np.asarray(src), dtype=torch.long)] * w(sign)
        rows[2] = (mu - twin).pow(2).sum(-1) / A
        sq = rows[2].sum() * A
        mirror = sq / (M * A)
        mirror_g = sq / M if mutation == "mirror_mean_over_B" else mirror
    imit = imit_g = zero
    imit_coeff = 0.0
    if imitation is not None:
        imit_coeff, target, mask, n_selected = imitation
        mask = torch.as_tensor(np.asarray(mask)).to(dtype)
        rows[5] = (mask * (mu - w(target)).pow(2)).sum(-1) * (M / float(n_selected))
        sq = rows[5].sum() * (float(n_selected) / M)
        imit = sq / float(n_selected)
        k = int((mask.sum(0) > 0).sum())
        imit_g = sq / float(M * k) if mutation == "imit_denominator_Bk" else imit
    entropy_penalty = -(0.5 + 0.5 * math.log(2.0 * math.pi) + torch.log(stds)).mean()
    total = ((1.01 if mutation == "ppo_x1.01" else 1.0) * actor + mirror_coeff * mirror_g + imit_coeff * imit_g
             + (2.0 if mutation == "entropy_x2" else 1.0) * entropy_coeff * entropy_penalty + (0.5 if mutation == "critic_half" else 1.0) * critic)
    total.backward()
    with torch.no_grad():
        approx_kl = ((ratio - 1.0) - logr).mean()
        clip_fraction = ((ratio - 1.0).abs() > clip).to(dtype).mean()
    scalars = np.array([float(x.detach()) for x in (actor_true, critic, mirror, approx_kl, clip_fraction, imit)], dtype=np.float64)
    grads = {n: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().to(torch.float64).numpy() for n, p in P.items()}
    extras = {i: r.detach().to(torch.float64).numpy() for i, r in rows.items()}      # per-row terms: scalar i is their mean over the rows
    extras["ratio"] = ratio.detach().to(torch.float64).numpy()
    return scalars, grads, extras


def ff_names():
    return [f"a_{n}" for n in FF_NET] + [f"c_{n}" for n in FF_NET]


def rnn_names():
    return [f"a_{n}" for n in RNN_NET] + [f"c_{n}" for n in RNN_NET]


def ff_reference(theta, xn, xm, act, old_logp, adv, ret, *, clip=0.2, mirror_coeff=0.4, entropy_coeff=0.0, learn_std=False, mirror_act=None,
                 imitation=None, dtype=torch.float64, mutation=None, want_rows=False):
    """Feed-forward minibatch.  theta: {name: float32 array} in torch layouts (a_w1 [H, D] ...); xn / xm [B, D] (xm None together with
    mirror_act: no mirror term); act [B, A]; old_logp / adv / ret [B]; mirror_act = (src, sign); imitation = (coeff, target [B, A], mask [B, A],
    n_selected) or None.  -> (scalars [6], {name: gradient}) (with want_rows also {i: the rows' terms of scalar i, "ratio": the rows' ratios})."""
    assert (xm is None) == (mirror_act is None)
    x = {False: torch.as_tensor(np.asarray(xn)).to(dtype), True: None if xm is None else torch.as_tensor(np.asarray(xm)).to(dtype)}
    s, g, rows = _loss_and_grad(theta, ff_names(), lambda p, twin: _mlp(x[twin], p), act, old_logp, adv, ret, clip=clip, mirror_coeff=mirror_coeff,
                                 entropy_coeff=entropy_coeff, learn_std=learn_std, mirror_act=mirror_act, imitation=imitation, dtype=dtype,
                                 mutation=mutation)
    return (s, g, rows) if want_rows else (s, g)


def rnn_reference(theta, xn, xm, reset, act, old_logp, adv, ret, *, clip=0.2, mirror_coeff=0.4, entropy_coeff=0.0, learn_std=False,
                  mirror_act=None, dtype=torch.float64, mutation=None, want_rows=False):
    """Recurrent minibatch on the selected columns: xn / xm [T, B, D], reset [T, B] bool (row 0 all True), act [T, B, A], old_logp / adv / ret
    [T, B]; the two-cell LSTM with its state zeroed at in-column episode starts, every (t, column) entry a sample."""
    assert (xm is None) == (mirror_act is None)
    x = {False: torch.as_tensor(np.asarray(xn)).to(dtype), True: None if xm is None else torch.as_tensor(np.asarray(xm)).to(dtype)}
    reset = torch.as_tensor(np.asarray(reset)).bool().clone()
    T, B = reset.shape
    if mutation == "resets_ignored":
        reset[1:] = False
    cut_at = T // 2 if mutation == "cell_state_cut" else None
    flat = lambda a: np.asarray(a).reshape(T * B, *np.asarray(a).shape[2:])
    net = lambda p, twin: _lstm(x[twin], reset, p, cut_at).reshape(T * B, -1)
    s, g, rows = _loss_and_grad(theta, rnn_names(), net, flat(act), flat(old_logp), flat(adv), flat(ret), clip=clip, mirror_coeff=mirror_coeff,
                                 entropy_coeff=entropy_coeff, learn_std=learn_std, mirror_act=mirror_act, imitation=None, dtype=dtype, mutation=mutation)
    return (s, g, rows) if want_rows else (s, g)


# ----------------------------------------------------------------------------- the bar
def _network(name):
    return "critic" if name.startswith("c_") else "actor"      # (the stds belong to the actor's group, as in the optimiser)


def rel_error(g, g64):
    """max |g - g64| / max |g64| of one tensor (inf where g64 is identically zero and g is not)"""
    top = float(np.abs(g64).max())
    err = float(np.abs(np.asarray(g, dtype=np.float64) - g64).max())
    return err / top if top > 0 else (0.0 if err == 0 else float("inf"))


def yardstick(g32, g64):
    """y(P) of every tensor whose float64 gradient is not identically zero: the float32 evaluation's distance to the float64 gradient"""
    return {n: rel_error(g32[n], g64[n]) for n in g64 if np.abs(g64[n]).max() > 0}


def bars(y):
    """bar(P) = MARGIN * max(y(P), median of y over the tensors of P's network)"""
    med = {net: float(np.median([v for n, v in y.items() if _network(n) == net])) for net in {_network(n) for n in y}}
    return {n: MARGIN * max(v, med[_network(n)]) for n, v in y.items()}


def scalar_bars(ref32, ref64):
    """The same style of bar for the loss scalars that are not identically zero, relative to |s64|; clip_fraction is a count over the rows: 1e-6
    absolute.  A scalar is the mean of M per-row terms whose float32 errors e_m have either sign, and |s32 - s64| = |sum e_m| / M is ONE draw of
    that cancelling sum, which comes out far below its own scale often enough: with the draw alone as the yardstick, the same reference in float32
    with its sums in another order missed 8 x it for 7 of 108 scalars (actor_loss, approx_kl: losses that cancel themselves) -- see
    tests/test_grad_reference.py::test_another_summation_order_stays_within_the_bars.  So the yardstick of a scalar is the larger of that draw
    and the scale it is drawn from, sqrt(sum e_m^2) / M, both from the reference's own float32 evaluation, never from a kernel."""
    (s32, _, r32), (s64, _, r64) = ref32, ref64
    y = {}
    for i in (0, 1, 2, 3, 5):
        if s64[i] != 0:
            spread = float(np.sqrt(np.sum((r32[i] - r64[i]) ** 2))) / len(r64[i])
            y[i] = max(abs(s32[i] - s64[i]), spread) / abs(s64[i])
    med = float(np.median(list(y.values())))
    return {i: MARGIN * max(v, med) for i, v in y.items()}


def compare(grads, stats, ref64, ref32):
    """Kernel gradient ``grads`` {name: array} and scalars ``stats`` [6] against the float64 reference (scalars, gradients), with the bars of the
    float32 yardstick ``ref32`` (both (scalars, gradients, rows) of a reference called with want_rows).  -> (worst error / bar, its name, worst
    error / y over the tensors with each tensor's OWN y(P) -- not floored by the median, so it may exceed MARGIN where the bar holds --, its
    name, failures: list of strings)."""
    s64, g64 = ref64[:2]
    s32, g32 = ref32[:2]
    y = yardstick(g32, g64)
    bar = bars(y)
    fails, worst, worst_raw = [], (0.0, ""), (0.0, "")
    for n in g64:
        if n not in y:
            if np.asarray(grads[n]).any():
                fails.append(f"{n}: the float64 gradient is identically zero, the kernel's is not")
            continue
        e = rel_error(grads[n], g64[n])
        worst = max(worst, (e / bar[n], n))
        worst_raw = max(worst_raw, (e / y[n], n))
        if e > bar[n]:
            fails.append(f"{n}: error {e:.3g} > bar {bar[n]:.3g} (y = {y[n]:.3g})")
    sb = scalar_bars(ref32, ref64)
    for i, name in enumerate(SCALARS):
        if i == 4:
            if abs(stats[4] - s64[4]) > 1e-6:
                fails.append(f"clip_fraction: {stats[4]!r} vs {s64[4]!r}")
        elif i not in sb:
            if stats[i] != 0:
                fails.append(f"{name}: the reference is identically zero, the kernel's is {stats[i]!r}")
        else:
            e = abs(float(stats[i]) - s64[i]) / abs(s64[i])
            worst = max(worst, (e / sb[i], name))
            if e > sb[i]:
                fails.append(f"{name}: error {e:.3g} > bar {sb[i]:.3g}")
    return worst[0], worst[1], worst_raw[0], worst_raw[1], fails


def rejection(grads, mutated64, ref64, ref32):
    """How far the kernel's gradient lies from a MUTATED reference, in units of the true reference's bar: max over the tensors"""
    g64 = ref64[1]
    bar = bars(yardstick(ref32[1], g64))
    out = 0.0
    for n, b in bar.items():
        top = float(np.abs(g64[n]).max())
        out = max(out, float(np.abs(np.asarray(grads[n], dtype=np.float64) - mutated64[1][n]).max()) / top / b)
    return out


# ----------------------------------------------------------------------------- inputs that put every branch of the head in play
TARGET_RATIOS = (0.5, 0.7, 0.79, 0.9, 1.0, 1.1, 1.21, 1.4, 2.0)      # below, inside and above the clip range 1 +- 0.2, none within 1e-3 of an edge
ZERO_EVERY, ZERO_AT = 16, 5


def design(M, rs):
    """Per minibatch position j < M: the target ratio (cycling through the nine TARGET_RATIOS) and the advantage (sign alternating with j, so
    that it also alternates from one cycle to the next; magnitude 0.3 .. 2; an exact zero at every position j % 16 == 5): every class {below,
    inside, above} x {adv > 0, adv < 0} and adv == 0 is populated within the first nine rows, twice within the first 22."""
    j = np.arange(M)
    target = np.asarray(TARGET_RATIOS)[j % 9]
    adv = np.where(j % 2 == 0, 1.0, -1.0) * rs.uniform(0.3, 2.0, size=M)
    adv[j % ZERO_EVERY == ZERO_AT] = 0.0
    return target, adv.astype(np.float32)


def class_counts(ratio, adv, clip=0.2):
    """rows per class of the head's branches, from the float64 ratios; asserts that no row sits within 1e-3 of a branch point"""
    ratio, adv = np.asarray(ratio).reshape(-1), np.asarray(adv).reshape(-1)
    assert np.abs(ratio - (1 - clip)).min() > 1e-3 and np.abs(ratio - (1 + clip)).min() > 1e-3, "a row sits on a clip edge"
    where = np.where(ratio < 1 - clip, 0, np.where(ratio > 1 + clip, 2, 1))
    out = {f"{w}/{s}": int(((where == i) & (adv > 0 if s == "adv>0" else adv < 0)).sum())
           for i, w in enumerate(("below", "inside", "above")) for s in ("adv>0", "adv<0")}
    out["adv==0"] = int((adv == 0).sum())
    return out


def _rollout_side(theta, names, mu, value, rs):
    """actions = mean + noise of about one std (rounded to float32 first), their float64 log-density, returns = value + noise"""
    stds = torch.as_tensor(np.asarray(theta["stds"])).double()
    act = (mu + stds * torch.as_tensor(rs.normal(size=tuple(mu.shape)))).float()
    z = (act.double() - mu) / stds
    logp = (-0.5 * z * z - torch.log(stds) - 0.5 * math.log(2.0 * math.pi)).sum(-1)
    ret = (value + torch.as_tensor(rs.normal(size=tuple(value.shape)))).float()
    return act, logp, ret


def ff_inputs(theta, xn, minibatches, rs):
    """Stored rows for a feed-forward handle: xn [R, D] float32 (as the kernels normalised it), minibatches = disjoint index arrays into the R rows.
    -> act [R, A], old_logp [R], adv [R], ret [R] float32 tensors; row minibatches[k][j] follows design()[j]."""
    d = lambda n: torch.as_tensor(np.asarray(theta[n])).double()
    x = torch.as_tensor(np.asarray(xn)).double()
    with torch.no_grad():
        mu = _mlp(x, {n: d(f"a_{n}") for n in FF_NET})
        v = _mlp(x, {n: d(f"c_{n}") for n in FF_NET})[:, 0]
    act, logp, ret = _rollout_side(theta, ff_names(), mu, v, rs)
    R = x.shape[0]
    target, adv = np.ones(R), rs.normal(size=R).astype(np.float32)
    for idx in minibatches:
        target[np.asarray(idx)], adv[np.asarray(idx)] = design(len(idx), rs)
    old_logp = (logp - torch.as_tensor(np.log(target))).float()
    return act, old_logp, torch.as_tensor(adv), ret


def rnn_inputs(theta, xn, reset, minibatches, rs):
    """The same for a recurrent handle: xn [T, N, D], reset [T, N] bool, minibatches = disjoint arrays of columns; minibatch row t * B + b (column
    minibatches[k][b]) follows design()[t * B + b].  -> act [T, N, A], old_logp / adv / ret [T, N]."""
    d = lambda n: torch.as_tensor(np.asarray(theta[n])).double()
    x, reset = torch.as_tensor(np.asarray(xn)).double(), torch.as_tensor(np.asarray(reset)).bool()
    T, N = reset.shape
    with torch.no_grad():
        mu = _lstm(x, reset, {n: d(f"a_{n}") for n in RNN_NET})
        v = _lstm(x, reset, {n: d(f"c_{n}") for n in RNN_NET})[..., 0]
    act, logp, ret = _rollout_side(theta, rnn_names(), mu, v, rs)
    target, adv = np.ones((T, N)), rs.normal(size=(T, N)).astype(np.float32)
    for cols in minibatches:
        cols = np.asarray(cols)
        t, a = design(T * len(cols), rs)
        target[:, cols], adv[:, cols] = t.reshape(T, len(cols)), a.reshape(T, len(cols))
    old_logp = (logp - torch.as_tensor(np.log(target))).float()
    return act, old_logp, torch.as_tensor(adv), ret


# ----------------------------------------------------------------------------- what the GPU tests of both handle kinds share
def outside_named_tensors(k):
    """bool [n_params] on the handle's device: True at every element of the flat vector that no named tensor's true extent covers (W1 columns
    obs_dim .. Dp, read-out rows act_dim .. Op, the critic's read-out rows 1 .. 3, the std pad slots)"""
    covered = torch.zeros(k.n_params, dtype=torch.bool, device=k.grad.device)
    for n in k._specs:
        k._view(covered, n).fill_(True)
    return ~covered


def check_gradient(label, k, ref, mutations, active, stats_scale=1.0):
    """The handle's ``grad`` and ``stats[:6]`` (after grad calls on a zeroed grad / stats, no apply) against ``ref(dtype=..., mutation=...)`` ->
    (scalars, gradients): every tensor and scalar within its bar, exact zeros where the float64 gradient is identically zero and outside the named
    tensors, every active mutation rejected by at least 10 bars.  Prints the case's worst error / y."""
    from tests.test_optimizer_gpu import _layout
    torch.cuda.synchronize()
    grads = {n: t.numpy() for n, t in k.get_tensors(k.grad).items()}
    stats = k.stats[:6].cpu().numpy().astype(np.float64)
    assert np.isfinite(stats).all() and all(np.isfinite(g).all() for g in grads.values())
    ref64, ref32 = ref(want_rows=True), ref(dtype=torch.float32, want_rows=True)
    worst, name, worst_raw, name_raw, fails = compare(grads, stats, ref64, ref32)
    rej = {m: rejection(grads, ref(mutation=m), ref64, ref32) for m in mutations if mutation_is_active(m, **active)}
    # the scalar bars bite too: each loss scalar the kernels report, taken 1 % too large, lies >= 10 bars from the reference
    sb = scalar_bars(ref32, ref64)
    rej_s = {SCALARS[i]: abs(1.01 * stats[i] - ref64[0][i]) / abs(ref64[0][i]) / b for i, b in sb.items()}
    print(f"GRADCHECK {label}: worst error / y {MARGIN * worst:.3g} ({name}) with y floored by its network's median, {worst_raw:.3g} ({name_raw}) over "
          f"each tensor's own y; negative controls " + ", ".join(f"{m} {v:.3g}" for m, v in rej.items()) +
          "; scalars x 1.01 " + ", ".join(f"{m} {v:.3g}" for m, v in rej_s.items()))
    assert not fails, fails
    # padding: everything outside the named tensors' true extents, and the std slots of a handle whose stds are not parameters
    bad = int(k.grad[outside_named_tensors(k)].count_nonzero())
    assert bad == 0, f"{bad} padding entries of the gradient are non-zero"
    off_std, off_critic, _ = _layout(k)
    assert not k.grad[off_std + k.act_dim:off_critic].any(), "std pad slots"
    if not k.learn_std:
        assert not k.grad[off_std:off_critic].any(), "the stds are not parameters: their gradient slots stay zero"
    for m, v in rej.items():
        assert v >= 10.0, f"negative control {m}: the kernel's gradient lies only {v:.3g} bars from the mutated reference"
    for m, v in rej_s.items():
        assert v >= 10.0, f"negative control {m} x 1.01: only {v:.3g} bars from the reference"
    return MARGIN * worst


def assert_classes(label, ratio, adv, need=2):
    counts = class_counts(ratio, adv)
    print(f"GRADCHECK {label}: rows per class {counts}")
    assert min(counts.values()) >= need, counts
