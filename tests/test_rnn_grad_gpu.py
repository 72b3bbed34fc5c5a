"""What lhw_rnn_grad leaves in ``grad`` and ``stats[:6]`` against float64 autograd through the two-cell LSTM (tests/ppo_grad_reference.py): one
grad_columns on a zeroed gradient, no apply().  The checks, the bar (8 x the float32 yardstick of the same reference, per tensor, floored by the
network's median) and the inputs are those of tests/test_ppo_grad_gpu.py; the minibatch is a scrambled subset of the N columns, episodes start
inside the columns (done values 1 .. 3), one column has no start and one starts an episode at its last step.  Negative controls of the recurrent
form: in-column resets ignored, and no gradient through the cell state across one step.  The path is asserted from last_grad_fused: the
whole-sequence strips, the same handle shape with them switched off, and a hidden width the strips do not cover.  ``learn_std`` (the dstd column
sums plus entropy_grad_kernel) has no other reference: the CPU oracle's recurrent form has no learnable stds.

The h256 case is the existing T = 3, B = 3 shape: nine rows cannot hold two rows of each of the seven classes, so there one row per class is
asserted; every other case asserts two.

Measured on an MI355X, worst error / y per path over its cases: first with y floored by its network's median, as in the bar (the bar is 8), then
over each tensor's OWN y(P), which the bar does not use alone.  The whole-sequence strips and the launch-per-step loops leave the same bits, so each
pair of cases measures the same:
    hidden 32, T = 24 (B = 33 and 5, mirror off / on)      4.91  c_whh2, B = 33 mirror off; 4.23 c_bout, B = 5 mirror on     own y 9.82  c_bout; 8.48 c_whh2
    hidden 64, T = 24 (B = 33 and 5, mirror off / on)      4.42  actor_loss, B = 33 mirror off; 4.40 approx_kl, mirror on    own y 8.03  c_bout
    hidden 256, T = 3, B = 3                               2.52  c_whh1                                                      own y 2.52  c_whh1
    hidden 48 (launch-per-step only), T = 12, B = 5        1.98  a_wih2                                                      own y 15.2  c_bout
    learnable stds, hidden 64, T = 24, B = 33              4.40  approx_kl                                                   own y 3.94  a_wih2
    two calls accumulating                                 2.06  c_bih1                                                      own y 3.33  c_wih1
Above 4, floored: y is the max-norm error of ONE float32 evaluation -- one draw; the reference in float32 with its sums in another order reaches
4.3 on the CPU (tests/test_grad_reference.py::test_another_summation_order_stays_within_the_bars), so 4 .. 5 is the spread of the yardstick.
actor_loss / approx_kl at B = 33: their yardstick is the scale of a sum of independent per-row errors, and along a column the log-probability's
errors are not independent (the carried state passes them on) -- a supposition.  Above 8 over the own y: c_bout is ONE number, its y one draw of
float32 roundoff, which is what the median in the bar is there for; c_whh2's own y (hidden 32, B = 33) lies below its network's median in that
case, and its error is 0.6 bars.
Negative controls, the smallest rejection over all cases, in bars: critic x 0.5 2.0e5, PPO term x 1.01 1.3e3, mirror mean over B 4.2e4, no min
1.3e5, entropy coefficient x 2 874, twin's gradient dropped 2.1e3, resets ignored 2.8e5, cell state cut at one step 9.3e4; a reported scalar
x 1.01: 222 (actor_loss).
"""
import numpy as np
import pytest
import torch

from tests import ppo_grad_reference as R
from tests.test_rnn_gpu import MIR_ACT, MIR_OBS

pytestmark = pytest.mark.gpu

D, A, ENTROPY = 37, 12, 0.01
UNCOVERED_HIDDEN = 48      # not a multiple of 32: outside the whole-sequence strips (as tests/test_lstm_seq_gpu.py picks it)


def _case(H, T, N, B, mirror, fused, learn_std=False, expect_fused=None):
    return dict(H=H, T=T, N=N, B=B, mirror=mirror, fused=fused, learn_std=learn_std, expect_fused=fused if expect_fused is None else expect_fused)


CASES = {}
for _H in (32, 64):
    for _B in (33, 5):
        for _m in (False, True):
            for _f in (1, 0):
                CASES[f"h{_H}-T24-B{_B}of40-{'mirror' if _m else 'nomirror'}-{'strips' if _f else 'per-step'}"] = _case(_H, 24, 40, _B, _m, _f)
for _f in (1, 0):
    CASES[f"h256-bt3-mirror-{'strips' if _f else 'per-step'}"] = _case(256, 3, 5, 3, True, _f)
    CASES[f"h64-T24-B33of40-mirror-std-{'strips' if _f else 'per-step'}"] = _case(64, 24, 40, 33, True, _f, learn_std=True)
CASES["h48-T12-B5of9-mirror-uncovered-width"] = _case(UNCOVERED_HIDDEN, 12, 9, 5, True, 1, expect_fused=0)


def _setup(c, monkeypatch, n_minibatches=1):
    from learninghumanoidwalking_amd.rnn_kernels import RnnKernels
    from oracle import ppo_oracle as po
    H, T, N, B = c["H"], c["T"], c["N"], c["B"]
    assert n_minibatches * B <= N
    monkeypatch.delenv("LHW_RNN_SEQ_FUSED", raising=False)
    kw = dict(mirror_obs=po.mirror_tables(MIR_OBS, [29, 30]), mirror_act=po.mirror_tables(MIR_ACT)) if c["mirror"] else {}
    k = RnnKernels(D, A, hidden=H, seq_len=T, seq_cols=B, rollout_rows=N, learn_std=c["learn_std"], entropy_coeff=ENTROPY if c["learn_std"] else 0.0, **kw)
    k.set_seq_fused(bool(c["fused"]))
    rs = np.random.default_rng(100 * H + T + B + c["mirror"])
    w = {}
    for n, t in k.get_tensors().items():
        scale = 0.1 if t.dim() == 1 else 1.0 / np.sqrt(t.shape[-1])      # non-zero biases, a read-out that is not scaled down
        w[n] = torch.tensor((rs.normal(size=tuple(t.shape)) * scale).astype(np.float32))
    w["stds"] = torch.tensor(np.linspace(0.15, 0.4, A).astype(np.float32))
    k.set_tensors(w)
    mean, std = rs.normal(size=D).astype(np.float32) * 0.3, (0.5 + rs.uniform(size=D)).astype(np.float32)
    k.set_obs_norm(mean, std)
    perm = rs.permutation(N)
    mbs = [perm[i * B:(i + 1) * B] for i in range(n_minibatches)]
    done = ((rs.uniform(size=(T, N)) < (0.3 if T < 6 else 0.12)) * rs.integers(1, 4, size=(T, N))).astype(np.uint8)
    for cols in mbs:
        done[:, cols[0]] = 0              # a column without an episode start inside it
        done[T - 2, cols[1]] = 3          # one that starts an episode at its last step
        done[0, cols[2]] = 1              # (and early ones, whatever the draw gave: every done value 1 .. 3 occurs inside the minibatch)
        if B > 3:
            done[1, cols[3]] = 2
    assert set(np.unique(done)) <= {0, 1, 2, 3}
    reset = np.ones((T, N), bool)
    reset[1:] = done[:-1] != 0
    obs = torch.tensor(rs.normal(size=(T * N, D)).astype(np.float32) * std + mean).cuda()
    xn, xm = k.normalize(obs)
    assert not xn[:, D:].any()
    theta = {n: t.numpy() for n, t in k.get_tensors().items()}
    xn_h = xn[:, :D].cpu().numpy().reshape(T, N, D)
    xm_h = xm[:, :D].cpu().numpy().reshape(T, N, D) if c["mirror"] else None
    act, old_logp, adv, ret = R.rnn_inputs(theta, xn_h, reset, mbs, rs)
    dev = [xn, xm if c["mirror"] else None, act.reshape(T * N, A).cuda().contiguous(), old_logp.reshape(-1).cuda(), adv.reshape(-1).cuda(),
           ret.reshape(-1).cuda(), torch.tensor(done).cuda()]

    def ref_of(i):
        cols = mbs[i]
        kwr = dict(entropy_coeff=ENTROPY if c["learn_std"] else 0.0, learn_std=c["learn_std"], mirror_act=kw.get("mirror_act"))
        return lambda **o: R.rnn_reference(theta, xn_h[:, cols], None if xm_h is None else xm_h[:, cols], reset[:, cols], act[:, cols],
                                           old_logp[:, cols], adv[:, cols], ret[:, cols], **kwr, **o)

    def run(i):
        k.grad_columns(T, N, *dev, torch.tensor(mbs[i].astype(np.int32)).cuda())
    return k, run, ref_of, adv, mbs


@pytest.mark.parametrize("case", list(CASES))
def test_column_minibatch_gradient_matches_float64_autograd(case, monkeypatch):
    c = CASES[case]
    k, run, ref_of, adv, mbs = _setup(c, monkeypatch)
    ref = ref_of(0)
    R.assert_classes(case, ref(want_rows=True)[2]["ratio"], adv[:, mbs[0]].numpy(), need=2 if c["T"] * c["B"] >= 22 else 1)
    k.grad.zero_()
    k.stats.zero_()
    run(0)
    torch.cuda.synchronize()
    assert k.last_grad_fused == c["expect_fused"], "the path this case is written for is the path that ran"
    R.check_gradient(case, k, ref, R.RNN_MUTATIONS, dict(mirror=c["mirror"], learn_std=c["learn_std"]))


def test_two_calls_accumulate_the_sum_of_two_column_sets(monkeypatch):
    """lhw_rnn_grad "accumulates grad, stats_dev[0..5]": two calls on two disjoint column sets without apply() leave the sum of the two references
    (whole-sequence strips, mirror on, learnable stds)."""
    c = _case(64, 24, 40, 5, True, 1, learn_std=True)
    k, run, ref_of, adv, mbs = _setup(c, monkeypatch, n_minibatches=2)
    for i in (0, 1):
        R.assert_classes(f"accumulate-rnn minibatch {i}", ref_of(i)(want_rows=True)[2]["ratio"], adv[:, mbs[i]].numpy())
    k.grad.zero_()
    k.stats.zero_()
    for i in (0, 1):
        run(i)
        torch.cuda.synchronize()
        assert k.last_grad_fused == 1, "the whole-sequence strips ran"

    def both(**o):
        a, b = ref_of(0)(**o), ref_of(1)(**o)
        out = (a[0] + b[0], {n: a[1][n] + b[1][n] for n in a[1]})
        # (with want_rows: the sum of two means over M rows each is the mean of the 2 M doubled terms)
        return out + ({i: 2.0 * np.concatenate([a[2][i], b[2][i]]) for i in a[2]},) if len(a) == 3 else out
    R.check_gradient("accumulate-rnn", k, both, R.RNN_MUTATIONS, dict(mirror=True, learn_std=True))
