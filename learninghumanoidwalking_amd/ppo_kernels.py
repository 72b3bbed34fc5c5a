"""Host handle over the on-device PPO kernels (include/lhw.h, `lhw_ppo_*`, `lhw_gae`).

torch owns the flat parameter / gradient / Adam-state tensors ("PyTorch-ROCm for parameter
storage"); every arithmetic step of the learner runs in liblhw.so.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import torch

from . import _lib

def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class _Kernels:
    """What the feed-forward and the LSTM handle share: the LhwPpoConfig (with the mirror tables it points to kept alive), the flat
    parameter / gradient / Adam vectors and the observation normalisation torch owns, tensor views into them, and the entry points
    that differ only in their prefix (``_API``: lhw_ppo or lhw_rnn).  A subclass creates its handle through ``create_args`` (what
    its ``_create`` entry point takes between the config and the handle) and fills ``_specs`` from its layout."""

    recurrent = False
    _API = "lhw_ppo"

    def __init__(self, obs_dim, act_dim, hidden, max_rows, create_args=(), *, device=0, learn_std=False, lr=3e-4, eps=1e-5,
                 clip=0.2, entropy_coeff=0.0, mirror_coeff=0.4, max_grad_norm=0.5, mirror_obs=None, mirror_act=None):
        if not torch.cuda.is_available():
            raise _lib.LhwError(-5, "no GPU visible: the PPO kernels have no CPU fallback")
        self.device = torch.device("cuda", device) if isinstance(device, int) else device
        self._L = _lib.lib()
        cfg = _lib.LhwPpoConfig()
        cfg.device = self.device.index or 0
        cfg.obs_dim, cfg.act_dim, cfg.hidden = obs_dim, act_dim, hidden
        cfg.learn_std, cfg.max_rows = int(learn_std), int(max_rows)
        cfg.lr, cfg.eps, cfg.clip = lr, eps, clip
        cfg.entropy_coeff, cfg.mirror_coeff, cfg.max_grad_norm = entropy_coeff, mirror_coeff, max_grad_norm
        self._keep = []
        if mirror_obs is not None:
            (os_, og), (as_, ag) = mirror_obs, mirror_act
            arrs = [np.ascontiguousarray(os_, np.int32), np.ascontiguousarray(og, np.float32),
                    np.ascontiguousarray(as_, np.int32), np.ascontiguousarray(ag, np.float32)]
            self._keep = arrs
            cfg.mirror_obs_src, cfg.mirror_obs_sign, cfg.mirror_act_src, cfg.mirror_act_sign = [a.ctypes.data for a in arrs]
        self.use_mirror = mirror_obs is not None
        self._h = ctypes.c_void_p()
        _lib.check(self._fn("create")(ctypes.byref(cfg), *create_args, ctypes.byref(self._h)))
        self.obs_dim, self.act_dim, self.hidden, self.max_rows, self.learn_std = obs_dim, act_dim, hidden, max_rows, learn_std
        self.eps = eps
        self.n_params = int(self._fn("param_count")(self._h))
        dev = self.device
        self.theta = torch.zeros(self.n_params, dtype=torch.float32, device=dev)
        self.grad = torch.zeros_like(self.theta)
        self.adam_m = torch.zeros_like(self.theta)
        self.adam_v = torch.zeros_like(self.theta)
        self.adam_step = 0
        self.stats = torch.zeros(16, dtype=torch.float32, device=dev)
        self._mom = torch.zeros(2, dtype=torch.float64, device=dev)
        self.obs_mean = torch.zeros(obs_dim, dtype=torch.float32, device=dev)
        self.obs_std = torch.ones(obs_dim, dtype=torch.float32, device=dev)

    def _fn(self, name):
        return getattr(self._L, f"{self._API}_{name}")

    def _layout(self, n):
        lay = (ctypes.c_int64 * n)()
        _lib.check(self._fn("layout")(self._h, lay))
        return [int(x) for x in lay]

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._fn("destroy")(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ---- parameter views in torch layouts (for init / checkpoints / the optimiser views / parity tests)
    def _view(self, flat, name):
        """Tensor `name` as a view into a flat [n_params] vector (theta, grad, adam_m, adam_v).  _specs[name] is (offset, length) or,
        for a matrix stored row-major with leading dimension ld, (offset, rows, ld, first column, columns)."""
        spec = self._specs[name]
        if len(spec) == 2:
            return flat[spec[0]:spec[0] + spec[1]]
        off, rows, ld, c0, cols = spec
        return flat[off:off + rows * ld].view(rows, ld)[:, c0:c0 + cols]

    def get_tensors(self, flat=None):
        flat = self.theta if flat is None else flat
        return {n: self._view(flat, n).detach().cpu().clone() for n in self._specs}

    def set_tensors(self, tensors: dict):
        for n, t in tensors.items():
            v = self._view(self.theta, n)
            v.copy_(torch.as_tensor(t, dtype=torch.float32).reshape(v.shape))

    def set_obs_norm(self, mean, std):
        self.obs_mean.copy_(torch.as_tensor(np.asarray(mean), dtype=torch.float32))
        self.obs_std.copy_(torch.as_tensor(np.asarray(std), dtype=torch.float32))

    # ---- kernels
    def normalize(self, obs, want_mirror=None):
        R = obs.shape[0]
        want_mirror = self.use_mirror if want_mirror is None else want_mirror
        xn = _lib.empty(R, self.Dp, dtype=torch.float32, device=self.device)
        xm = _lib.empty(R, self.Dp, dtype=torch.float32, device=self.device) if want_mirror else None
        _lib.check(self._fn("normalize")(self._h, _p(obs), R, _p(self.obs_mean), _p(self.obs_std), _p(xn), _p(xm), self._stream()))
        return xn, xm

    def gae(self, rew, val, done, vterm, vfinal, gamma, lam):
        T, N = rew.shape
        ret = _lib.empty(T, N, dtype=torch.float32, device=self.device)
        adv = _lib.empty(T, N, dtype=torch.float32, device=self.device)
        _lib.check(self._L.lhw_gae(T, N, _p(rew), _p(val), _p(done), _p(vterm), _p(vfinal), float(gamma), float(lam),
                                   _p(ret), _p(adv), self._stream()))
        return ret, adv

    def moments(self, x):
        _lib.check(self._L.lhw_moments(_p(x), x.numel(), _p(self._mom), self._stream()))
        return self._mom

    def standardize(self, x, stats3, eps):
        """x <- (x - mean) / (std + eps) from the device-resident {sum, sum of squares, count} (no host round trip)."""
        assert stats3.dtype == torch.float64 and stats3.numel() == 3 and stats3.is_cuda
        _lib.check(self._L.lhw_standardize(_p(x), x.numel(), _p(stats3), float(eps), self._stream()))

    def scale_shift(self, x, mean, inv):
        _lib.check(self._L.lhw_scale_shift(_p(x), x.numel(), float(mean), float(inv), self._stream()))

    def apply(self, grad_scale=1.0):
        self.adam_step += 1
        _lib.check(self._fn("apply")(self._h, _p(self.theta), _p(self.grad), _p(self.adam_m), _p(self.adam_v),
                                     self.adam_step, float(grad_scale), self._stream()))

    def debug_grad_sqnorms(self):
        """(actor, critic) squared gradient norms the last optimiser step clipped with (synchronises the device)."""
        out = (ctypes.c_float * 2)()
        _lib.check(self._fn("debug_grad_sqnorms")(self._h, out))
        return float(out[0]), float(out[1])


# Observation rows wider than 64 padded columns (obs_history_len > 1) through the wide instantiations of the LDS-resident strip kernels --
# inference, the critic's values behind the resident rollout and the update's forward / loss / backward launches -- instead of one GEMM per
# layer (lhw_ppo_debug_set_strip_wide).  LHW_STRIP_WIDE = 0 | 1 overrides; read once per handle.  Same bits either way; the default follows
# the project's A/B rule: True only once every run with the strips lies below every run without them.
STRIP_WIDE_DEFAULT = False
# fp16 operands (--fp16, --infer-fp16) through the fp16 strip kernels -- one forward and one backward launch per network in the update, one forward
# launch in inference -- instead of one fp16 GEMM per layer (lhw_ppo_debug_set_strip_fp16; narrow shapes, fp16 storage).  LHW_STRIP_FP16 = 0 | 1
# overrides; read once per handle.  Same bits either way; the default follows the same A/B rule.
STRIP_FP16_DEFAULT = False


class PpoKernels(_Kernels):
    """Flat-parameter actor/critic (D -> H -> H -> A | 1, ReLU) living on one GPU."""

    TENSORS = ["a_w1", "a_b1", "a_w2", "a_b2", "a_w3", "a_b3", "stds", "c_w1", "c_b1", "c_w2", "c_b2", "c_w3", "c_b3"]

    def __init__(self, obs_dim, act_dim, *, hidden=256, max_rows=4096, **kw):
        super().__init__(obs_dim, act_dim, hidden, max_rows, **kw)
        lay = self._layout(15)
        self.offsets = lay[:13]
        self.Dp, self.Op = lay[13], lay[14]
        o = dict(zip(self.TENSORS, self.offsets))
        H, D, A, Dp = hidden, obs_dim, act_dim, self.Dp

        def net(p, rows):      # (the output layer is stored with Op / 4 rows, the view shows the true ones)
            return {f"{p}_w1": (o[f"{p}_w1"], H, Dp, 0, D), f"{p}_b1": (o[f"{p}_b1"], H), f"{p}_w2": (o[f"{p}_w2"], H, H, 0, H),
                    f"{p}_b2": (o[f"{p}_b2"], H), f"{p}_w3": (o[f"{p}_w3"], rows, H, 0, H), f"{p}_b3": (o[f"{p}_b3"], rows)}
        self._specs = {**net("a", A), "stds": (o["stds"], A), **net("c", 1)}
        self.strip_wide = os.environ.get("LHW_STRIP_WIDE", "1" if STRIP_WIDE_DEFAULT else "0") != "0"
        _lib.check(self._L.lhw_ppo_debug_set_strip_wide(self._h, int(self.strip_wide)))
        self.set_strip_fp16(os.environ.get("LHW_STRIP_FP16", "1" if STRIP_FP16_DEFAULT else "0") != "0")

    def set_strip_fp16(self, on=True):
        """fp16 operands run the fp16 strip kernels where the plan allows (lhw_ppo_debug_set_strip_fp16); same bits as the per-layer fp16 GEMMs."""
        _lib.check(self._L.lhw_ppo_debug_set_strip_fp16(self._h, int(bool(on))))
        self.strip_fp16 = bool(on)

    @property
    def last_grad_fused(self):
        """1 if the last grad_minibatch / step_minibatch ran the train strip launches, 0 if forward, loss kernel and backward."""
        return int(self._L.lhw_ppo_debug_last_grad_fused(self._h))

    PLAN_FIELDS = ("fp16_operands", "fp16_storage", "fwd_strip", "bwd_strip", "train_strip", "mask_bits", "wide", "streams",
                   "infer_fp16_operands", "infer_strips", "policy_step", "critic_copies", "actor_copies")

    def plan(self, B=None, imitation=False):
        """Which kernels the handle's calls launch (lhw_ppo_debug_plan): the plan of a grad_minibatch on B rows (default max_rows), with an
        imitation term armed or not, then that of ``forward`` and the rollout bracket.  fwd_strip / bwd_strip: 1 actor | 2 critic."""
        out = (ctypes.c_int32 * len(self.PLAN_FIELDS))()
        _lib.check(self._L.lhw_ppo_debug_plan(self._h, int(self.max_rows if B is None else B), int(bool(imitation)), out))
        return dict(zip(self.PLAN_FIELDS, (int(v) for v in out)))

    def set_tensors(self, tensors: dict):
        # theta changes: a rollout bracket opened on the old weights (its [in][out] copies, the resident rollout's actor view) is void
        self.end_rollout()
        super().set_tensors(tensors)

    def set_inference_fp16(self, on=True):
        """Rollout inference (``forward``) with fp16 operands on the fp16 MFMA; the update stays float32."""
        _lib.check(self._L.lhw_ppo_set_inference_dtype(self._h, int(bool(on))))
        self.inference_fp16 = bool(on)

    def set_update_fp16(self, on=True):
        """Every GEMM of the update (``grad_minibatch``) with fp16 operands on the fp16 MFMA, float32 accumulation; master
        weights, loss and Adam stay float32 (BASELINE config 5, together with ``set_inference_fp16``)."""
        _lib.check(self._L.lhw_ppo_set_update_dtype(self._h, int(bool(on))))
        self.update_fp16 = bool(on)

    # ---- kernels
    def forward(self, obs, *, seed=0, env_id_base=0, counter=0, deterministic=False, want_actor=True, want_value=True,
                mu=None, act=None, logp=None, value=None, ws_row=0, want_mu=True):
        N = obs.shape[0]
        dev = self.device
        if want_actor:
            if want_mu:      # (the rollout needs only the sampled action and its log-density: one strided copy less per step)
                mu = _lib.empty(N, self.act_dim, dtype=torch.float32, device=dev) if mu is None else mu
            else:
                mu = None
            act = _lib.empty(N, self.act_dim, dtype=torch.float32, device=dev) if act is None else act
            logp = _lib.empty(N, dtype=torch.float32, device=dev) if logp is None else logp
        if want_value:
            value = _lib.empty(N, dtype=torch.float32, device=dev) if value is None else value
        _lib.check(self._L.lhw_ppo_forward_at(self._h, _p(self.theta), _p(obs), N, _p(self.obs_mean), _p(self.obs_std),
                                              int(seed) & (2**64 - 1), int(env_id_base), int(counter), int(deterministic), int(ws_row),
                                              _p(mu) if (want_actor and mu is not None) else None, _p(act) if want_actor else None,
                                              _p(logp) if want_actor else None, _p(value) if want_value else None,
                                              self._stream()))
        return mu, act, logp, value

    def begin_rollout(self):
        """theta is frozen until end_rollout(): the strip kernel's weight copies are made once (on the current stream) instead of
        in every policy step (lhw_ppo_begin_rollout)."""
        _lib.check(self._L.lhw_ppo_begin_rollout(self._h, _p(self.theta), self._stream()))

    def end_rollout(self):
        _lib.check(self._L.lhw_ppo_end_rollout(self._h))

    def rollout_policy(self, *, seed=0, counter=0, deterministic=False):
        """The frozen actor as the resident rollout (BatchedEnv.rollout -> lhw_env_rollout) evaluates it inside the stepper's
        wavefronts; valid inside a begin_rollout() bracket.  Returns None where the in-wave policy step does not apply (shapes outside
        the strip kernels): the caller keeps the launch-per-step pipeline.  With fp16 inference the view carries fp16_operands = 1: the
        in-wave policy step then rounds its operands to fp16 like the launch-per-step fp16 GEMMs do, but sums in another order -- that
        resident rollout is float32-rounding-close (~1e-6) to the launch-per-step one, not bitwise (the float32 policy step is bitwise)."""
        view = _lib.LhwRolloutPolicy()
        rc = self._L.lhw_ppo_rollout_policy(self._h, _p(self.theta), _p(self.obs_mean), _p(self.obs_std), int(seed) & (2**64 - 1),
                                            int(counter) & 0xFFFFFFFF, int(bool(deterministic)), ctypes.byref(view))
        if rc == -4:      # LHW_ERR_UNSUPPORTED
            return None
        _lib.check(rc)
        return view

    def grad_minibatch(self, xn, xm, act, old_logp, adv, ret, idx, imitation=None):
        """``imitation`` = (coeff, target [B, A] f32, mask [B, A] u8, n_selected): the imitation term of this minibatch
        (rows in ``idx`` order), see lhw_ppo_set_imitation."""
        B = idx.numel()
        if imitation is not None:
            coeff, target, mask, count = imitation
            assert target.shape == (B, self.act_dim) and mask.shape == (B, self.act_dim) and mask.dtype == torch.uint8
            self._imit_keep = (target.contiguous(), mask.contiguous())      # must outlive the asynchronous kernel
            _lib.check(self._L.lhw_ppo_set_imitation(self._h, _p(self._imit_keep[0]), _p(self._imit_keep[1]), float(coeff), int(count)))
        _lib.check(self._L.lhw_ppo_grad(self._h, _p(self.theta), _p(self.grad), _p(xn), _p(xm), _p(act), _p(old_logp),
                                        _p(adv), _p(ret), _p(idx), B, _p(self.stats), self._stream()))

    def step_minibatch(self, xn, xm, act, old_logp, adv, ret, idx, grad_scale=1.0):
        """grad_minibatch + apply as ONE hipGraph launch (lhw_ppo_step: single process, no imitation term).  Must run on a torch stream
        other than the default one (a legacy default stream cannot be captured: the library then makes the two calls eagerly)."""
        self.adam_step += 1
        _lib.check(self._L.lhw_ppo_step(self._h, _p(self.theta), _p(self.grad), _p(self.adam_m), _p(self.adam_v), _p(xn), _p(xm), _p(act),
                                        _p(old_logp), _p(adv), _p(ret), _p(idx), idx.numel(), _p(self.stats), self.adam_step,
                                        float(grad_scale), self._stream()))


def reference_init(obs_dim, act_dim, hidden=256, init_std=0.223, generator_seed=None):
    """Initial weights with exactly the RNG consumption of the reference's constructors
    (reference rl/policies/actor.py:122-158, critic.py:15-39, base.py:5-22): three nn.Linear per
    net (default init draws), then normc (weight ~ N(0,1), rows scaled to unit L2 norm, bias 0),
    actor mean layer x0.01 -- so that the same torch seed gives the reference's initial weights."""
    import torch.nn as nn

    # the draws come from the CPU default generator, seeded here and restored afterwards; the CUDA generators are left alone
    # (torch.manual_seed would reseed them too)
    with torch.random.fork_rng(devices=[]):
        if generator_seed is not None:
            torch.default_generator.manual_seed(int(generator_seed))
        return _reference_init_draw(obs_dim, act_dim, hidden, init_std)


def _reference_init_draw(obs_dim, act_dim, hidden, init_std):
    import torch.nn as nn

    def net(out_dim, scale_out):
        layers = [nn.Linear(obs_dim, hidden), nn.Linear(hidden, hidden), nn.Linear(hidden, out_dim)]
        for l in layers:
            l.weight.data.normal_(0, 1)
            l.weight.data *= 1 / torch.sqrt(l.weight.data.pow(2).sum(1, keepdim=True))
            l.bias.data.fill_(0)
        if scale_out is not None:
            layers[2].weight.data.mul_(scale_out)
        return layers

    a = net(act_dim, 0.01)
    c = net(1, None)
    out = {}
    for pre, ls in (("a", a), ("c", c)):
        for k, l in enumerate(ls, 1):
            out[f"{pre}_w{k}"] = l.weight.data.clone()
            out[f"{pre}_b{k}"] = l.bias.data.clone()
    out["stds"] = init_std * torch.ones(act_dim)
    return out
