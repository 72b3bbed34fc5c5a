"""The critic of a recurrent rollout in one launch on the GPU (lhw_rnn_values; csrc/lhw_mlp_strip.hip: lstm_seq_value_strip_kernel) against
the calls it replaces -- per control step lhw_rnn_forward(commit = 1) for V(s_t) and lhw_rnn_forward(commit = 0) for V(terminal
observation), and one more for the final value: every value and the critic state left behind BITWISE equal, which pins the kernel's
fmaf chains, its normalisation and its read-out to the MFMA GEMMs' bits.  Then RecurrentRollout with the switch LHW_RNN_SEQ_CRITIC on and
off, on both collection paths.  GPU twin of tests/test_emu_lstm_values.py (SIMT emulator), whose rollout construction it uses."""
import os
import subprocess
import sys

import pytest
import torch

from tests.test_emu_lstm_values import done_cases, done_flags

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET = ("wih1", "whh1", "bih1", "bhh1", "wih2", "whh2", "bih2", "bhh2", "wout", "bout")
SENTINEL = 7.0


def _kernels(D, A, rows, seed, hidden):
    from learninghumanoidwalking_amd.rnn_kernels import RnnKernels
    k = RnnKernels(D, A, hidden=hidden, seq_len=4, seq_cols=4, rollout_rows=rows)
    g = torch.Generator().manual_seed(seed)
    H = hidden
    for pre, O in (("a", A), ("c", 1)):
        shapes = [(4 * H, D), (4 * H, H), (4 * H,), (4 * H,), (4 * H, H), (4 * H, H), (4 * H,), (4 * H,), (O, H), (O,)]
        scale = [2.0 / D ** 0.5, 2.0 / H ** 0.5, 0.1, 0.1, 2.0 / H ** 0.5, 2.0 / H ** 0.5, 0.1, 0.1, 2.0 / H ** 0.5, 0.05]
        k.set_tensors({f"{pre}_{n}": torch.randn(*s, generator=g) * c for n, s, c in zip(NET, shapes, scale)})
    k.set_tensors({"stds": torch.full((A,), 0.223)})
    k.set_obs_norm(torch.randn(D, generator=g).numpy() * 0.1, 0.5 + torch.rand(D, generator=g).numpy())
    return k


def _rollout(D, T, N, seed):
    """obs [T + 1][N][D], term_obs (the next observation except where the episode ended: fresh data there), done, reset0 -- on the device"""
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn(T + 1, N, D, generator=g) * 1.5
    done = torch.from_numpy(done_flags(T, N))
    tob = obs[1:].clone()
    ended = done != 0
    tob[ended] = torch.randn(int(ended.sum()), D, generator=g) * 1.5
    reset0 = (torch.arange(N) % 3 == 1).to(torch.uint8)
    return obs.cuda(), tob.cuda(), done.cuda(), reset0.cuda()


def _warm_up(k, D, N):
    """a few committed steps, so that the critic's state is not zero"""
    g = torch.Generator().manual_seed(2)
    for i in range(3):
        k.forward((torch.randn(N, D, generator=g)).cuda(), commit=True, want_actor=False)


def test_done_pattern_of_the_gpu_cases_has_every_case():
    assert all(done_cases(done_flags(6, 40)).values())


@pytest.mark.parametrize("hidden", [64, 256])
def test_values_is_bitwise_the_forward_loop(hidden):
    D, A, T, N = 37, 12, 6, 40
    ka, kb = _kernels(D, A, N, 3, hidden), _kernels(D, A, N, 3, hidden)
    _warm_up(ka, D, N)
    _warm_up(kb, D, N)
    obs, tob, done, reset0 = _rollout(D, T, N, 5)
    out = {m: dict(val=torch.full((T, N), SENTINEL, device="cuda"), vterm=torch.full((T, N), SENTINEL, device="cuda"),
                   vfinal=torch.full((N,), SENTINEL, device="cuda")) for m in "ab"}
    assert ka.values(obs, tob, done, reset0, out["a"]["val"], out["a"]["vterm"], out["a"]["vfinal"]) is True
    reset = reset0
    for t in range(T):
        kb.forward(obs[t], reset=reset, commit=True, want_actor=False, value=out["b"]["val"][t])
        kb.forward(tob[t], commit=False, want_actor=False, value=out["b"]["vterm"][t])
        reset = (done[t] != 0).to(torch.uint8)
    kb.forward(obs[T], commit=False, want_actor=False, value=out["b"]["vfinal"])
    torch.cuda.synchronize()
    for key in ("val", "vterm", "vfinal"):
        x, y = out["a"][key], out["b"][key]
        assert torch.isfinite(x).all() and (x != SENTINEL).all(), key
        assert torch.equal(x, y), (key, (x != y).nonzero()[:8].tolist(), float((x - y).abs().max()))
    ended = (done != 0)[:-1]
    assert (out["a"]["vterm"][:-1][ended] != out["a"]["val"][1:][ended]).all()      # the terminal values are values of their own
    # the state: one more committed step (with the resets of the last step) gives the same values on both handles
    g = torch.Generator().manual_seed(9)
    for i in range(2):
        x = torch.randn(N, D, generator=g).cuda()
        va = ka.forward(x, reset=reset if i == 0 else None, commit=True, want_actor=False)[3]
        vb = kb.forward(x, reset=reset if i == 0 else None, commit=True, want_actor=False)[3]
        assert torch.equal(va, vb), i
    # ... and so does a second call of the entry itself, from the state the first one left
    obs2, tob2, done2, _ = _rollout(D, 4, N, 6)
    v2 = {m: (torch.zeros(4, N, device="cuda"), torch.zeros(4, N, device="cuda"), torch.zeros(N, device="cuda")) for m in "ab"}
    assert ka.values(obs2, tob2, done2, None, *v2["a"]) and kb.values(obs2, tob2, done2, None, *v2["b"])
    for x, y in zip(v2["a"], v2["b"]):
        assert torch.equal(x, y)


def test_values_declines_an_uncovered_hidden_width_and_writes_nothing():
    D, A, T, N = 37, 12, 4, 5
    k = _kernels(D, A, N, 3, 48)
    obs, tob, done, reset0 = _rollout(D, T, N, 5)
    val, vterm, vfinal = (torch.full(s, SENTINEL, device="cuda") for s in ((T, N), (T, N), (N,)))
    assert k.values(obs, tob, done, reset0, val, vterm, vfinal) is False
    torch.cuda.synchronize()
    assert (val == SENTINEL).all() and (vterm == SENTINEL).all() and (vfinal == SENTINEL).all()


_CHILD = r"""
import sys, torch
from types import SimpleNamespace
sys.path.insert(0, sys.argv[1])
from learninghumanoidwalking_amd.envs import ENVIRONMENTS
from learninghumanoidwalking_amd.ppo import PPO, RecurrentRollout
mode, critic, out = sys.argv[2], sys.argv[3], sys.argv[4]
a = SimpleNamespace(gamma=0.99, lam=0.95, lr=3e-4, eps=1e-5, entropy_coeff=0.0, clip=0.2, minibatch_size=16, epochs=1, max_traj_len=12,
                    num_procs=64, num_envs=97, max_grad_norm=0.5, mirror_coeff=0.4, eval_freq=10**9, recurrent=True, imitate=None,
                    learn_std=False, std_dev=1.0, no_mirror=True, continued=None, logdir=out + "_log", device_index=0, lstm_hidden=int(sys.argv[5]))
algo = PPO(ENVIRONMENTS["jvrc_walk"], a, seed=5)
# rollouts of 9 control steps on envs that truncate at 12, and a policy noisy enough to make the robot fall before that
ro = RecurrentRollout(algo.env, algo.kernels, 9, seed=77)
res = {}
for n in range(2):
    ro.collect()
    assert ro.last_mode == mode, ro.last_mode
    assert ro.last_critic_mode == critic, ro.last_critic_mode
    for name in ("obs", "act", "logp", "rew", "done", "val", "vterm", "vfinal"):
        res[f"{name}{n}"] = getattr(ro, name).cpu().clone()
torch.save(res, out)
"""


@pytest.mark.parametrize("mode,hidden", [("steps", 64), ("resident", 256)])
def test_recurrent_rollout_is_bitwise_the_same_with_the_sequence_critic(tmp_path, mode, hidden):
    """RecurrentRollout under LHW_RNN_SEQ_CRITIC=1 and =0, each in a fresh child process: every stored buffer of two consecutive
    collect() calls (the critic's state and the episode-start flags carry from the first into the second)."""
    script = tmp_path / "child.py"
    script.write_text(_CHILD)
    res = {}
    for sw, critic in (("1", "sequence"), ("0", "steps")):
        out = tmp_path / f"{mode}_{sw}.pt"
        env = dict(os.environ, LHW_ROLLOUT_MODE=mode, LHW_RNN_SEQ_CRITIC=sw)
        r = subprocess.run([sys.executable, str(script), ROOT, mode, critic, str(out), str(hidden)], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        res[sw] = torch.load(out)
    assert res["1"].keys() == res["0"].keys() and len(res["1"]) == 16
    for key in res["1"]:
        assert torch.equal(res["1"][key], res["0"][key]), key
    d0, d1 = res["1"]["done0"], res["1"]["done1"]
    assert (d0[:-1] != 0).any() and (d1[:-1] != 0).any(), "no episode end inside a rollout"
    slabs = [(d != 0)[:, b:b + 32].any(dim=1) for d in (d0, d1) for b in range(0, d.shape[1], 32)]
    assert any((~s).any() for s in slabs) and any(s.any() for s in slabs), "both branches of the vterm rule (a slab-step with / without an episode end) must run"
