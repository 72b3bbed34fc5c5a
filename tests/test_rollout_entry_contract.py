"""What the five resident-rollout entry points refuse, and with which code (include/lhw.h: lhw_env_rollout, _task_inputs,
_step_task_inputs, _history, _lstm), on the SIMT emulator: one table of bad calls, each tried through every entry point it applies to.
A refused call launches nothing: every output buffer is still zero and the env state is what it was.  The table does not say which
code wins where two errors meet, and leaves the NULL-env calls out."""
import ctypes

import numpy as np
import pytest

from tests import emu
from tests.test_rollout_lstm import NumpyLstmActor
from tests.test_rollout_resident import NumpyActor, _buffers

ARG, UNSUPPORTED = -1, -4      # LHW_ERR_ARG, LHW_ERR_UNSUPPORTED
N, T = 3, 2
# (entry point, history_len): lhw_env_rollout_history is tried with a history and with history_len = 1, which forwards to lhw_env_rollout's kernels
ENTRIES = [("rollout", 1), ("task_inputs", 1), ("step_task_inputs", 1), ("history", 2), ("history", 1), ("lstm", 1)]
BUFFERS = ("obs", "act", "logp", "tob", "rew", "done")


def _cap(entry, H):
    from learninghumanoidwalking_amd import _lib as product
    return product.ROLLOUT_HISTORY_MAX_OBS_PAD if (entry, H) == ("history", 2) else 64


def _cases(entry, H):
    """(name, env, overrides, expected code): an override names an argument of the call (None: passed as NULL; tin / stin True: passed
    where the entry point makes them optional) or `pol.<field>` of the policy view (a value, or a function of the valid one)"""
    env = "step" if entry == "step_task_inputs" else "walk"      # (lhw_env_rollout_step_task_inputs takes stepping envs only)
    c = [("first < 0", env, dict(first=-1), ARG), ("count = 0", env, dict(count=0), ARG), ("count < 0", env, dict(count=-2), ARG),
         ("first + count > N", env, dict(first=1, count=N), ARG), ("T = 0", env, dict(T=0), ARG), ("T < 0", env, dict(T=-3), ARG),
         ("null policy", env, dict(pol=None), ARG)]
    c += [(f"null {k}", env, {k: None}, ARG) for k in BUFFERS]
    if entry == "lstm":
        c.append(("null reset0", env, dict(reset0=None), ARG))
    if entry in ("task_inputs", "step_task_inputs"):
        c.append(("null tin", env, dict(tin=None), ARG))
    if entry == "step_task_inputs":
        c.append(("null stin", env, dict(stin=None), ARG))
    if entry == "history":
        c += [("history_len = 0", env, dict(H=0), ARG), ("history_len < 0", env, dict(H=-1), ARG)]
    if entry in ("history", "lstm"):
        c.append(("stin without tin", "step", dict(stin=True), ARG))
    if entry in ("step_task_inputs", "history", "lstm"):
        c.append(("stin on a non-stepping env", "walk", dict(tin=True, stin=True), UNSUPPORTED))
    c.append(("cartpole env", "cartpole", {}, UNSUPPORTED))
    cap = _cap(entry, H)
    c += [("hidden 128", env, {"pol.hidden": 128}, UNSUPPORTED), ("obs_dim one less", env, {"pol.obs_dim": lambda d: d - 1}, UNSUPPORTED),
          ("obs_dim of twice the history", env, {"pol.obs_dim": lambda d: 2 * d}, UNSUPPORTED), ("act_dim 11", env, {"pol.act_dim": 11}, UNSUPPORTED),
          ("act_pad 20", env, {"pol.act_pad": 20}, UNSUPPORTED), ("act_pad 14", env, {"pol.act_pad": 14}, UNSUPPORTED),
          ("obs_pad above the capacity", env, {"pol.obs_pad": cap + 4}, UNSUPPORTED),
          ("obs_pad no multiple of 4", env, {"pol.obs_pad": lambda p: p + 2}, UNSUPPORTED)]
    if entry == "lstm":
        c += [("state_rows < N", env, {"pol.state_rows": N - 1}, UNSUPPORTED), ("h1_ld 258", env, {"pol.h1_ld": 258}, UNSUPPORTED),
              ("h1_ld 252", env, {"pol.h1_ld": 252}, UNSUPPORTED)]
    return c


@pytest.fixture(scope="module")
def envs():
    from learninghumanoidwalking_amd.envs import CartpoleSpec
    from learninghumanoidwalking_amd.envs.jvrc_step import JvrcStepSpec
    from learninghumanoidwalking_amd.envs.jvrc_walk import JvrcWalkSpec
    out = {}
    for name, spec in (("walk", JvrcWalkSpec()), ("step", JvrcStepSpec()), ("cartpole", CartpoleSpec())):
        e = emu.make_emulated(spec, N, seed=5, max_traj_len=2)
        e.reset()
        out[name] = e
    yield out
    for e in out.values():
        e.close()


_POLICIES = {}


def _policy(entry, H, env):
    """a valid policy view of the entry point's kind for this env (cartpole: the walking env's shapes -- the call is refused before they matter)"""
    D, A = (env.obs_dim, env.act_dim) if env.task != 0 else (37, 12)
    key = (entry == "lstm", H * D, A)
    if key not in _POLICIES:
        _POLICIES[key] = NumpyLstmActor(D, A, N, seed=3) if entry == "lstm" else NumpyActor(H * D, A, seed=3)
    return _POLICIES[key]


def _call(entry, H, env, over, rew_terms=True):
    """one call of the entry point with `over` applied to otherwise valid arguments -> (return code, buffers)"""
    from learninghumanoidwalking_amd import _lib as product
    L = emu.lib()
    H = over.get("H", H)
    Hb = max(H, 1)
    D, A = (env.obs_dim, env.act_dim) if env.task != 0 else (37, 12)
    pol = _policy(entry, Hb, env)
    view = type(pol.view).from_buffer_copy(pol.view)
    for k, v in over.items():
        if k.startswith("pol."):
            setattr(view, k[4:], v(getattr(view, k[4:])) if callable(v) else v)
    b = _buffers(T, N, Hb * D, A)
    b["obs"][0, :, :env.obs.shape[1]] = env.obs.numpy()
    reset0 = np.ones(N, np.uint8)
    tin = np.zeros((T, N, product.TASK_INPUT_DIM))
    stin = np.zeros((T, N, product.STEP_TASK_INPUT_DIM))
    ptr = lambda k, a: None if (k in over and over[k] is None) else a.ctypes.data
    a = dict(first=0, count=N, T=T)
    a.update({k: v for k, v in over.items() if k in a})
    head = [env._h, None if ("pol" in over) else ctypes.byref(view), a["first"], a["count"], a["T"]]
    bufs = [ptr(k, b[k]) for k in BUFFERS] + [env.rew_terms.data_ptr() if rew_terms else None]
    want_tin = entry in ("task_inputs", "step_task_inputs") or over.get("tin") is True
    want_stin = entry == "step_task_inputs" or over.get("stin") is True
    ptin = ptr("tin", tin) if want_tin else None
    pstin = ptr("stin", stin) if want_stin else None
    if entry == "rollout":
        rc = L.lhw_env_rollout(*head, *bufs, None)
    elif entry == "task_inputs":
        rc = L.lhw_env_rollout_task_inputs(*head, *bufs, ptin, None)
    elif entry == "step_task_inputs":
        rc = L.lhw_env_rollout_step_task_inputs(*head, *bufs, ptin, pstin, None)
    elif entry == "history":
        rc = L.lhw_env_rollout_history(*head, H, *bufs, ptin, pstin, None)
    else:
        rc = L.lhw_env_rollout_lstm(*head, *bufs, ptr("reset0", reset0), ptin, pstin, None)
    b["tin"], b["stin"] = tin, stin
    return rc, b


ALL = [pytest.param(entry, H, *case, id=f"{entry}{'' if entry != 'history' else H}-{case[0]}") for entry, H in ENTRIES for case in _cases(entry, H)]


@pytest.mark.parametrize("entry,H,name,env_name,over,code", ALL)
def test_refused_call_returns_its_code_and_launches_nothing(envs, entry, H, name, env_name, over, code):
    env = envs[env_name]
    before = env.get_state()
    rc, b = _call(entry, H, env, over)
    assert rc == code, (rc, emu.lib().lhw_last_error())
    assert not b["obs"][1:].any()
    for k in ("act", "logp", "tob", "rew", "done", "tin", "stin"):
        assert not b[k].any(), k
    for x, y in zip(before, env.get_state()):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("entry,H", ENTRIES)
def test_rew_terms_may_be_null(envs, entry, H):
    env = envs["step" if entry == "step_task_inputs" else "walk"]
    rc, b = _call(entry, H, env, {}, rew_terms=False)
    assert rc == 0, emu.lib().lhw_last_error()
    assert b["act"].any() and b["obs"][T].any()
