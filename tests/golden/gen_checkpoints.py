"""Generates tests/golden/checkpoints/ with the REFERENCE's own policy classes (only possible where a reference checkout exists;
the fixtures are committed so tests/test_checkpoint.py runs anywhere).  Run: python tests/golden/gen_checkpoints.py REFERENCE_DIR

* ff.npz / lstm.npz: the inputs (obs, obs_mean, obs_std), what the reference's Gaussian_FF_Actor / FF_V (Gaussian_LSTM_Actor /
  LSTM_V) computed after unpickling OUR checkpoint files of those inputs, and the attribute names the unpickled objects carry.
* ref_actor_3.pt / ref_critic_3.pt, ref_lstm_actor_9.pt / ref_lstm_critic_9.pt: checkpoint files written by the reference itself.
"""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "checkpoints")

from learninghumanoidwalking_amd import checkpoint as ck  # noqa: E402
from tests.test_checkpoint import _lstm_tensors, _tensors  # noqa: E402

_NAMES = ("def names(m):\n"
          "    return sorted(k for k in vars(m) if not k.startswith('_') and k != 'training') + sorted(m._modules) + "
          "sorted(m._parameters) + sorted(m._buffers)\n")


def _run(code):
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def ff(ref, tmp):
    g = torch.Generator().manual_seed(11)
    om, osd, obs = torch.randn(37, generator=g) * 0.1, torch.rand(37, generator=g) + 0.5, torch.randn(5, 37, generator=g)
    a, c = os.path.join(tmp, "actor_0.pt"), os.path.join(tmp, "critic_0.pt")
    ck.save_reference_checkpoint(_tensors(), om, osd, True, a, c)
    torch.save(obs, os.path.join(tmp, "obs.pt"))
    _run("import sys, torch; sys.path.insert(0, %r)\n" % ref + _NAMES +
         "from rl.policies.actor import Gaussian_FF_Actor; from rl.policies.critic import FF_V\n"
         "p = torch.load(%r, weights_only=False); v = torch.load(%r, weights_only=False)\n"
         "assert type(p) is Gaussian_FF_Actor and type(v) is FF_V, (type(p), type(v))\n"
         "obs = torch.load(%r)\n"
         "torch.save((p(obs, deterministic=True).detach(), v(obs).detach(), p.distribution(obs).stddev.detach(), names(p), names(v)), %r)\n"
         "torch.manual_seed(5); p = Gaussian_FF_Actor(37, 12, init_std=0.2, learn_std=False); v = FF_V(37)\n"
         "p.obs_mean = torch.zeros(37); p.obs_std = torch.ones(37); v.obs_mean = p.obs_mean; v.obs_std = p.obs_std\n"
         "torch.save(p, %r); torch.save(v, %r)\n"
         % (a, c, os.path.join(tmp, "obs.pt"), os.path.join(tmp, "out.pt"), os.path.join(OUT, "ref_actor_3.pt"), os.path.join(OUT, "ref_critic_3.pt")))
    mu, val, sd, na, nc = torch.load(os.path.join(tmp, "out.pt"))
    np.savez(os.path.join(OUT, "ff.npz"), obs=obs.numpy(), obs_mean=om.numpy(), obs_std=osd.numpy(), mu=mu.numpy(), val=val.numpy(),
             sd=sd.numpy(), actor_names=np.array(na), critic_names=np.array(nc))


def lstm(ref, tmp):
    g = torch.Generator().manual_seed(12)
    om, osd, obs = torch.randn(37, generator=g) * 0.1, torch.rand(37, generator=g) + 0.5, torch.randn(6, 3, 37, generator=g)
    a, c = os.path.join(tmp, "lstm_actor_0.pt"), os.path.join(tmp, "lstm_critic_0.pt")
    ck.save_recurrent_checkpoint(_lstm_tensors(), om, osd, False, a, c)
    torch.save(obs, os.path.join(tmp, "lstm_obs.pt"))
    _run("import sys, torch; sys.path.insert(0, %r)\n" % ref + _NAMES +
         "from rl.policies.actor import Gaussian_LSTM_Actor; from rl.policies.critic import LSTM_V\n"
         "p = torch.load(%r, weights_only=False); v = torch.load(%r, weights_only=False)\n"
         "assert type(p) is Gaussian_LSTM_Actor and type(v) is LSTM_V, (type(p), type(v))\n"
         "obs = torch.load(%r)\n"
         "torch.save((p(obs, deterministic=True).detach(), v(obs).detach(), names(p), names(v)), %r)\n"
         "torch.manual_seed(9); q = Gaussian_LSTM_Actor(37, 12, layers=(32, 32), init_std=0.2); w = LSTM_V(37, layers=(32, 32))\n"
         "q.obs_mean = torch.zeros(37); q.obs_std = torch.ones(37); w.obs_mean = q.obs_mean; w.obs_std = q.obs_std\n"
         "torch.save(q, %r); torch.save(w, %r)\n"
         % (a, c, os.path.join(tmp, "lstm_obs.pt"), os.path.join(tmp, "lstm_out.pt"), os.path.join(OUT, "ref_lstm_actor_9.pt"),
            os.path.join(OUT, "ref_lstm_critic_9.pt")))
    mu, val, na, nc = torch.load(os.path.join(tmp, "lstm_out.pt"))
    np.savez(os.path.join(OUT, "lstm.npz"), obs=obs.numpy(), obs_mean=om.numpy(), obs_std=osd.numpy(), mu=mu.numpy(), val=val.numpy(),
             actor_names=np.array(na), critic_names=np.array(nc))


if __name__ == "__main__":
    import tempfile
    ref = sys.argv[1]
    os.makedirs(OUT, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        ff(ref, tmp)
        lstm(ref, tmp)
    print("wrote", sorted(os.listdir(OUT)))
