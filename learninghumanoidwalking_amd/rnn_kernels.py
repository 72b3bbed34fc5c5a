"""ctypes view of the recurrent (LSTM) PPO kernels (include/lhw.h, lhw_rnn_*): Gaussian_LSTM_Actor / LSTM_V of the
reference (rl/policies/actor.py:191-286, critic.py:52-112) as one flat float32 parameter vector on the GPU."""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from .ppo_kernels import _Kernels, _p


class RnnKernels(_Kernels):
    """Two stacked LSTM cells + linear read-out for the actor and for the critic.

    Tensor names (torch layouts): ``{a,c}_wih1 [4H, D]``, ``_whh1 [4H, H]``, ``_bih1``, ``_bhh1``, ``_wih2 [4H, H]``,
    ``_whh2``, ``_bih2``, ``_bhh2``, ``_wout [A | 1, H]``, ``_bout``, and ``stds``."""

    recurrent = True
    _API = "lhw_rnn"

    def __init__(self, obs_dim, act_dim, *, hidden=256, seq_len=400, seq_cols=64, rollout_rows=4096, **kw):
        super().__init__(obs_dim, act_dim, hidden, rollout_rows, (int(seq_len), int(seq_cols), int(rollout_rows)), **kw)
        self.seq_len, self.seq_cols = seq_len, seq_cols
        self.offsets = self._layout(19)
        self.Dp, self.Op = self.offsets[17], self.offsets[18]
        self._specs = {**self._blocks("a"), "stds": (self.offsets[8], act_dim), **self._blocks("c")}
        self.TENSORS = list(self._specs)      # (in layout order, like PpoKernels.TENSORS)

    def _blocks(self, net):
        """name -> (offset, rows, ld, col0, cols) of every torch-layout tensor of one network inside theta."""
        H, D, Dp = self.hidden, self.obs_dim, self.Dp
        base = 0 if net == "a" else 9
        o = self.offsets[base:base + 8]
        out_rows = self.act_dim if net == "a" else 1
        K1 = Dp + H
        return {
            f"{net}_wih1": (o[0], 4 * H, K1, 0, D), f"{net}_whh1": (o[0], 4 * H, K1, Dp, H), f"{net}_bih1": (o[1], 4 * H), f"{net}_bhh1": (o[2], 4 * H),
            f"{net}_wih2": (o[3], 4 * H, 2 * H, 0, H), f"{net}_whh2": (o[3], 4 * H, 2 * H, H, H), f"{net}_bih2": (o[4], 4 * H), f"{net}_bhh2": (o[5], 4 * H),
            f"{net}_wout": (o[6], out_rows, H, 0, H), f"{net}_bout": (o[7], out_rows),
        }

    # ---- kernels
    def forward(self, obs, *, reset=None, seed=0, env_id_base=0, counter=0, deterministic=False, commit=True, want_actor=True,
                want_value=True, mu=None, act=None, logp=None, value=None):
        N, dev = obs.shape[0], self.device
        if want_actor:
            mu = _lib.empty(N, self.act_dim, dtype=torch.float32, device=dev) if mu is None else mu
            act = _lib.empty(N, self.act_dim, dtype=torch.float32, device=dev) if act is None else act
            logp = _lib.empty(N, dtype=torch.float32, device=dev) if logp is None else logp
        if want_value:
            value = _lib.empty(N, dtype=torch.float32, device=dev) if value is None else value
        _lib.check(self._L.lhw_rnn_forward(self._h, _p(self.theta), _p(obs), N, _p(self.obs_mean), _p(self.obs_std), _p(reset),
                                           int(seed) & (2**64 - 1), int(env_id_base), int(counter), int(deterministic), int(commit),
                                           _p(mu) if want_actor else None, _p(act) if want_actor else None,
                                           _p(logp) if want_actor else None, _p(value) if want_value else None, self._stream()))
        return mu, act, logp, value

    def values(self, obs, term_obs, done, reset0, val, vterm=None, vfinal=None) -> bool:
        """The critic over a stored rollout in one launch (lhw_rnn_values): ``obs [T + 1, N, D]`` raw observations, ``term_obs [T, N, D]``,
        ``done [T, N]`` uint8, ``reset0 [N]`` uint8 or None.  Bitwise what ``forward(obs[t], reset=..., commit=True, want_actor=False)``,
        ``forward(term_obs[t], commit=False, ...)`` per step and ``forward(obs[T], commit=False, ...)`` write to ``val [T, N]``,
        ``vterm [T, N]`` (None together with ``term_obs``) and ``vfinal [N]`` (may be None), and the critic state they leave.
        Returns False, with nothing written, where the kernel does not cover the critic's shape: the caller keeps those calls."""
        T, N = int(done.shape[0]), int(done.shape[1])
        assert obs.shape[0] == T + 1 and obs.shape[1] == N and obs.is_contiguous() and done.is_contiguous() and val.is_contiguous()
        assert (term_obs is None) == (vterm is None) and all(x is None or x.is_contiguous() for x in (term_obs, vterm, vfinal, reset0))
        rc = self._L.lhw_rnn_values(self._h, _p(self.theta), _p(obs), _p(term_obs), _p(done), _p(reset0), T, N, _p(self.obs_mean), _p(self.obs_std),
                                    _p(val), _p(vterm), _p(vfinal), self._stream())
        if rc == -4:      # LHW_ERR_UNSUPPORTED
            return False
        _lib.check(rc)
        return True

    def rollout_policy(self, *, seed=0, counter=0, deterministic=False):
        """The frozen LSTM actor as the resident rollout (BatchedEnv.rollout_lstm -> lhw_env_rollout_lstm) evaluates it inside the
        stepper's wavefronts: [in][out] weight copies made on the current stream, and this handle's own actor state buffers -- the ones
        ``forward(commit=True)`` advances -- which the rollout reads and writes.  Valid until theta changes (``apply``, ``set_tensors``).
        Returns None where the in-wave step does not apply (hidden width other than 256): the caller keeps the launch-per-step path."""
        view = _lib.LhwRolloutLstmPolicy()
        rc = self._L.lhw_rnn_rollout_policy(self._h, _p(self.theta), _p(self.obs_mean), _p(self.obs_std), int(seed) & (2**64 - 1),
                                            int(counter) & 0xFFFFFFFF, int(bool(deterministic)), ctypes.byref(view), self._stream())
        if rc == -4:      # LHW_ERR_UNSUPPORTED
            return None
        _lib.check(rc)
        return view

    def grad_columns(self, T, N, xn, xm, act, old_logp, adv, ret, done, cols):
        """BPTT over columns ``cols`` (int32 device tensor) of the time-major [T][N] rollout."""
        _lib.check(self._L.lhw_rnn_grad(self._h, _p(self.theta), _p(self.grad), int(T), int(N), _p(xn), _p(xm), _p(act), _p(old_logp),
                                        _p(adv), _p(ret), _p(done), _p(cols), int(cols.numel()), _p(self.stats), self._stream()))

    def set_seq_fused(self, on):
        """A/B switch: the forward and BPTT time loops of ``grad_columns`` as one whole-sequence strip launch each per network (``True``)
        or as four launches per time step (``False``).  Same bits either way; a new handle takes ``LHW_RNN_SEQ_FUSED`` from the environment."""
        _lib.check(self._L.lhw_rnn_debug_set_seq_fused(self._h, int(bool(on))))

    @property
    def last_grad_fused(self):
        """1 if the last ``grad_columns`` ran the whole-sequence strip kernels, 0 if the launch-per-step loops (shape not covered, or switched off)."""
        return int(self._L.lhw_rnn_debug_last_grad_fused(self._h))


def reference_init_lstm(obs_dim, act_dim, hidden=256, init_std=0.2, generator_seed=None):
    """Initial weights with the RNG consumption of the reference's recurrent constructors (reference
    rl/policies/actor.py:191-232, critic.py:52-66, base.py:5-22): per network two nn.LSTMCell (default uniform init, not
    touched by normc_fn) and one nn.Linear read-out, then normc on the Linear (actor read-out x0.01); actor first."""
    import torch.nn as nn
    # the draws come from the CPU default generator, seeded here and restored afterwards; the CUDA generators are left alone
    # (torch.manual_seed would reseed them too)
    with torch.random.fork_rng(devices=[]):
        if generator_seed is not None:
            torch.default_generator.manual_seed(int(generator_seed))
        return _reference_init_lstm_draw(obs_dim, act_dim, hidden, init_std)


def _reference_init_lstm_draw(obs_dim, act_dim, hidden, init_std):
    import torch.nn as nn

    def net(out_dim, scale_out):
        cells = [nn.LSTMCell(obs_dim, hidden), nn.LSTMCell(hidden, hidden)]
        lin = nn.Linear(hidden, out_dim)
        lin.weight.data.normal_(0, 1)
        lin.weight.data *= 1 / torch.sqrt(lin.weight.data.pow(2).sum(1, keepdim=True))
        lin.bias.data.fill_(0)
        if scale_out is not None:
            lin.weight.data.mul_(scale_out)
        return cells, lin

    out = {}
    for pre, (cells, lin) in (("a", net(act_dim, 0.01)), ("c", net(1, None))):
        for k, cell in enumerate(cells, 1):
            out[f"{pre}_wih{k}"], out[f"{pre}_whh{k}"] = cell.weight_ih.data.clone(), cell.weight_hh.data.clone()
            out[f"{pre}_bih{k}"], out[f"{pre}_bhh{k}"] = cell.bias_ih.data.clone(), cell.bias_hh.data.clone()
        out[f"{pre}_wout"], out[f"{pre}_bout"] = lin.weight.data.clone(), lin.bias.data.clone()
    out["stds"] = init_std * torch.ones(act_dim)
    return out
