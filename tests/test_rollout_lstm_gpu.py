"""The resident rollout for LSTM actors on the GPU (lhw_env_rollout_lstm; csrc/lhw_humanoid_rollout.hip: lstm_policy_step) against the
launch-per-step LSTM path it replaces (T x { lhw_rnn_forward ; lhw_env_step }): every stored value BITWISE equal, which also pins the
in-wave v_fma_f32 chains to the bits of the MFMA GEMMs.  Reference: RolloutWorker.sample with a recurrent policy,
/root/reference/rl/workers/rollout_worker.py:130-190.  GPU twin of tests/test_rollout_lstm.py (SIMT emulator)."""
import ctypes
import os
import subprocess
import sys
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET = ("wih1", "whh1", "bih1", "bhh1", "wih2", "whh2", "bih2", "bhh2", "wout", "bout")


def _kernels(D, A, rows, seed, hidden=256):
    from learninghumanoidwalking_amd.rnn_kernels import RnnKernels
    k = RnnKernels(D, A, hidden=hidden, seq_len=4, seq_cols=4, rollout_rows=rows)
    g = torch.Generator().manual_seed(seed)
    H = hidden
    shapes = [(4 * H, D), (4 * H, H), (4 * H,), (4 * H,), (4 * H, H), (4 * H, H), (4 * H,), (4 * H,), (A, H), (A,)]
    scale = [2.0 / D ** 0.5, 2.0 / H ** 0.5, 0.1, 0.1, 2.0 / H ** 0.5, 2.0 / H ** 0.5, 0.1, 0.1, 2.0 / H ** 0.5, 0.05]
    k.set_tensors({f"a_{n}": torch.randn(*s, generator=g) * c for n, s, c in zip(NET, shapes, scale)})
    k.set_tensors({"stds": torch.full((A,), 0.223)})
    k.set_obs_norm(torch.randn(D, generator=g).numpy() * 0.1, 0.5 + torch.rand(D, generator=g).numpy())
    return k


def _hip():
    """the HIP runtime this process has loaded (torch's), for a strided device-to-device copy from a raw pointer"""
    with open("/proc/self/maps") as f:
        path = next(line.split()[-1] for line in f if "libamdhip64" in line)
    hip = ctypes.CDLL(path)
    hip.hipMemcpy2D.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int]
    hip.hipMemcpy2D.restype = ctypes.c_int
    return hip


def _state(view, N):
    """copies of the four actor state arrays behind a view's pointers: h1, h2, c1, c2 ([N][256] each, rows `ld` floats apart)"""
    torch.cuda.synchronize()
    hip, out = _hip(), []
    for ptr, ld in ((view.h1, view.h1_ld), (view.h2, view.h2_ld), (view.c1, 256), (view.c2, 256)):
        t = torch.empty(N, 256, dtype=torch.float32, device="cuda")
        assert hip.hipMemcpy2D(t.data_ptr(), 256 * 4, ptr, ld * 4, 256 * 4, N, 3) == 0      # 3: hipMemcpyDeviceToDevice
        out.append(t.cpu())
    return out


@pytest.mark.parametrize("deterministic", [False, True])
def test_debug_lstm_policy_step_is_bitwise_lhw_rnn_forward(deterministic):
    """(a) the plain reference launch == lhw_rnn_forward's actor (three MFMA GEMMs, two cell kernels, the sampler), commit = 1, over ten
    steps with episode starts on random rows: mu, act, logp and the handle's state.  Pins the fmaf chain order to the MFMA GEMM."""
    from learninghumanoidwalking_amd import _lib
    D, A, N = 37, 12, 77
    ka, kb = _kernels(D, A, N, 3), _kernels(D, A, N, 3)
    L = _lib.lib()
    g = torch.Generator().manual_seed(11)
    view = kb.rollout_policy(seed=99, counter=0, deterministic=deterministic)
    assert view is not None
    y = torch.zeros(N, view.act_pad, device="cuda")
    for t in range(10):
        obs = (torch.randn(N, D, generator=g) * 1.5).cuda()
        reset = (torch.rand(N, generator=g) < (1.0 if t == 0 else 0.2)).to(torch.uint8).cuda()
        mu, act, logp, _ = ka.forward(obs, reset=reset, seed=99, env_id_base=5, counter=40 + t, deterministic=deterministic, commit=True, want_value=False)
        act2, logp2 = torch.zeros_like(act), torch.zeros_like(logp)
        _lib.check(L.lhw_debug_lstm_policy_step(ctypes.byref(view), obs.data_ptr(), N, reset.data_ptr(), 5, 40 + t, y.data_ptr(), act2.data_ptr(),
                                                logp2.data_ptr(), None))
        torch.cuda.synchronize()
        assert torch.equal(mu, y[:, :A]), t
        assert torch.equal(act, act2) and torch.equal(logp, logp2), t
        va = ka.rollout_policy(seed=99, counter=0, deterministic=deterministic)
        for x, z in zip(_state(va, N), _state(view, N)):
            assert torch.equal(x, z), t
    assert deterministic == bool(torch.equal(mu, act))


@pytest.mark.parametrize("env_name", ["jvrc_walk", "h1", "h1_walk", "jvrc_step"])
def test_lstm_resident_rollout_is_bitwise_the_per_step_reference(env_name, monkeypatch):
    """(b) the emulator test's comparison on the hardware: lhw_env_rollout_lstm against T x { lhw_debug_lstm_policy_step ; env step }, odd
    batch, truncations inside the rollout, a non-zero reset0 on a non-zero state, a second rollout continuing from the first, armed term
    statistics giving the bits of unarmed, and (jvrc_step) the job queue."""
    from learninghumanoidwalking_amd import _lib
    from learninghumanoidwalking_amd.envs import ENVIRONMENTS
    L = _lib.lib()
    N, T = 97, 9
    spec = ENVIRONMENTS[env_name]()
    D, A = spec.obs_dim, spec.act_dim

    def run(mode):
        if mode == "queue":
            monkeypatch.setenv("LHW_ROLLOUT_SLOTS", "16")
            monkeypatch.setenv("LHW_ROLLOUT_CHUNK", "4")
        else:
            monkeypatch.delenv("LHW_ROLLOUT_SLOTS", raising=False)
            monkeypatch.delenv("LHW_ROLLOUT_CHUNK", raising=False)
        env = spec.make_batched(N, seed=3, max_traj_len=5)
        if mode == "armed":
            env.enable_term_stats(True)
        k = _kernels(D, A, N, 7)
        dev = env.device
        # a non-zero state to start from: two warm-up steps of the handle itself
        g = torch.Generator().manual_seed(2)
        for i in range(2):
            k.forward((torch.randn(N, D, generator=g)).cuda(), seed=1, counter=i, want_value=False)
        reset0 = (torch.rand(N, generator=g) < 0.5).to(torch.uint8).cuda()
        out = []
        obs0 = env.reset().clone()
        counter = 100
        for n in range(2):
            b = dict(obs=torch.zeros(T + 1, N, D, device=dev), act=torch.zeros(T, N, A, device=dev), logp=torch.zeros(T, N, device=dev),
                     tob=torch.zeros(T, N, D, device=dev), rew=torch.zeros(T, N, device=dev), done=torch.zeros(T, N, dtype=torch.uint8, device=dev))
            b["obs"][0] = obs0
            view = k.rollout_policy(seed=99, counter=counter)
            if mode == "steps":
                y = torch.zeros(N, view.act_pad, device=dev)
                reset = reset0
                for t in range(T):
                    _lib.check(L.lhw_debug_lstm_policy_step(ctypes.byref(view), b["obs"][t].data_ptr(), N, reset.data_ptr(), 0, counter + t, y.data_ptr(),
                                                            b["act"][t].data_ptr(), b["logp"][t].data_ptr(), None))
                    env.step(b["act"][t], obs_out=b["obs"][t + 1], term_obs_out=b["tob"][t], rew_out=b["rew"][t], done_out=b["done"][t])
                    reset = (b["done"][t] != 0).to(torch.uint8)
            else:
                assert env.rollout_lstm(view, T, b["obs"], b["act"], b["logp"], b["tob"], b["rew"], b["done"], reset0)
                assert env.last_rollout_queued() == (mode == "queue")
            torch.cuda.synchronize()
            out.append({k_: v.cpu() for k_, v in b.items()})
            out[-1]["state"] = _state(view, N)
            obs0, reset0, counter = b["obs"][T].clone(), (b["done"][T - 1] != 0).to(torch.uint8), counter + T
        q, v = env.get_state()
        return out, q, v

    modes = ["steps", "resident", "armed"] + (["queue"] if env_name == "jvrc_step" else [])
    res = {m: run(m) for m in modes}
    ref, qa, va = res["steps"]
    assert (ref[0]["done"][:-1] != 0).any(), "no episode end, hence no state reset, inside the rollout"
    for m in modes[1:]:
        got, q, v = res[m]
        for ra, rb in zip(ref, got):
            for key in ("obs", "act", "logp", "tob", "rew", "done"):
                assert torch.equal(ra[key], rb[key]), (m, key)
            for x, z in zip(ra["state"], rb["state"]):
                assert torch.equal(x, z), m
        np.testing.assert_array_equal(qa, q)
        np.testing.assert_array_equal(va, v)


_CHILD = r"""
import json, sys, torch
from types import SimpleNamespace
sys.path.insert(0, sys.argv[1])
from learninghumanoidwalking_amd.envs import ENVIRONMENTS
from learninghumanoidwalking_amd.ppo import PPO, RecurrentRollout
what, mode, out = sys.argv[2], sys.argv[3], sys.argv[4]
a = SimpleNamespace(gamma=0.99, lam=0.95, lr=3e-4, eps=1e-5, entropy_coeff=0.0, clip=0.2, minibatch_size=16, epochs=1, max_traj_len=12,
                    num_procs=64, num_envs=64 if what == "train" else 97, max_grad_norm=0.5, mirror_coeff=0.4, eval_freq=10**9, recurrent=True,
                    imitate=None, learn_std=False, std_dev=0.223, no_mirror=what != "train", continued=None, logdir=out + "_log", device_index=0,
                    lstm_hidden=int(sys.argv[5]))
algo = PPO(ENVIRONMENTS["jvrc_walk"], a, seed=5)
res = {}
if what == "collect":
    # rollouts of 9 control steps on envs that truncate at 12: episodes end at steps 11 and 23 of the run, INSIDE the second and third
    # rollout (the learner's own rollout is as long as an episode, so its truncations would all fall on a rollout's last step)
    ro = RecurrentRollout(algo.env, algo.kernels, 9, seed=77)
    for n in range(3):
        ro.collect()
        assert ro.last_mode == mode, ro.last_mode
        for name in ("obs", "act", "logp", "rew", "done", "val", "vterm", "vfinal"):
            res[f"{name}{n}"] = getattr(ro, name).cpu().clone()
else:
    for itr in range(2):
        algo.iterate(itr)
        assert algo.rollout.last_mode == mode, algo.rollout.last_mode
    res["theta"] = algo.kernels.theta.cpu().clone()
torch.save(res, out)
"""


def _child(tmp_path, what, mode, hidden=256):
    out = tmp_path / f"{what}_{mode}.pt"
    script = tmp_path / "child.py"
    script.write_text(_CHILD)
    env = dict(os.environ, LHW_ROLLOUT_MODE=mode)
    r = subprocess.run([sys.executable, str(script), ROOT, what, mode, str(out), str(hidden)], capture_output=True, text=True, timeout=900, env=env)
    return r, out


@pytest.mark.parametrize("what", ["collect", "train"])
def test_recurrent_rollout_modes_agree_bitwise_in_fresh_processes(tmp_path, what):
    """(c) RecurrentRollout under LHW_ROLLOUT_MODE=steps and =resident, each in a fresh child process: every buffer after collect() --
    val, vterm and vfinal included -- over three rollouts, and the weights after two full --recurrent PPO iterations on jvrc_walk."""
    res = {}
    for mode in ("steps", "resident"):
        r, out = _child(tmp_path, what, mode)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        res[mode] = torch.load(out)
    assert res["steps"].keys() == res["resident"].keys() and len(res["steps"]) > 0
    for key in res["steps"]:
        assert torch.equal(res["steps"][key], res["resident"][key]), key
    if what == "collect":      # state resets inside a rollout, not only at its first step
        assert (res["steps"]["done1"][:-1] != 0).any() and (res["steps"]["done2"][:-1] != 0).any()


def test_resident_mode_with_an_uncovered_hidden_width_raises_and_names_the_reason(tmp_path):
    """(d) LHW_ROLLOUT_MODE=resident with a 32-unit LSTM: no silent fall-back"""
    r, _ = _child(tmp_path, "collect", "resident", hidden=32)
    assert r.returncode != 0
    assert "LHW_ROLLOUT_MODE=resident" in r.stderr and "hidden width 256" in r.stderr and "32" in r.stderr
