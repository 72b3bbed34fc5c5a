"""lhw_render_scene on the GPU against the float64 ray caster of tests/render_scene_oracle.py (the cases of tests/test_render_scene.py
where the device can differ from the emulator: ballots over three passes, the LDS hand-off between passes, per-lane layer lists, the
dword output path), the recording rollout of the stepping env, and frames of its record with terrain and markers."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from learninghumanoidwalking_amd import _lib, markers
from learninghumanoidwalking_amd.render import Renderer
from tests import render_scene_checks as S
from tests.test_render_scene import guarded

pytestmark = pytest.mark.gpu


def make(gtype, size, rgba, W, H, **settings):
    return Renderer.from_geoms(gtype, size, rgba, W, H, device=0, **settings)


@pytest.mark.parametrize("name,min_cover", [("layers_seven", None), ("grid130", 0.05), ("dynamic_three", None), ("single_cone_rot", 0.05)])
def test_scene_against_the_oracle(name, min_cover):
    images = S.check_against_oracle(make, name, min_cover=min_cover)
    if name == "grid130":
        assert sorted(np.unique(images[1][images[1] >= 0] // 8).tolist()) == list(range(130))
    if name == "layers_seven":
        assert (images[3] == 2).any()


def test_clipped_tiles_write_inside_the_image_only():
    c = S.case("odd_layers")
    raw, per, out = guarded(c["W"], c["H"], device="cuda")
    images = S.draw(make, "odd_layers", out=out)
    for r, k in zip(raw, per):
        assert (r[c["W"] * c["H"] * k:] == 0xA5).all()
    S.check_against_oracle(make, "odd_layers", images=images, min_cover=0.05)


def _ppo(env_name, N=4, T=12, seed=4):
    from learninghumanoidwalking_amd.envs import ENVIRONMENTS
    from learninghumanoidwalking_amd.ppo import PPO
    args = SimpleNamespace(gamma=0.99, lam=0.95, lr=3e-4, eps=1e-5, entropy_coeff=0.0, clip=0.2, minibatch_size=N * T, epochs=1,
                           max_traj_len=T, num_procs=N, num_envs=N, max_grad_norm=0.5, mirror_coeff=0.4, eval_freq=10**9,
                           recurrent=False, imitate=None, learn_std=False, std_dev=0.223, no_mirror=False, continued=None,
                           logdir="/tmp/lhw_test_scene", device_index=0)
    return PPO(ENVIRONMENTS[env_name], args, seed=seed)


@functools.lru_cache(maxsize=None)
def _stepping_record():
    """(spec, model, record of the recording rollout, the resident rollout's arrays from the same seed)"""
    algo = _ppo("jvrc_step")
    algo.rollout.record_terrain = True
    algo.sample_parallel_with_workers()
    ro = algo.rollout
    assert ro.last_mode == "recorded"
    rec = dict(obs=ro.obs.cpu().numpy(), act=ro.act.cpu().numpy(), rew=ro.rew.cpu().numpy(), done=ro.done.cpu().numpy(), tin=ro.tin_all.cpu().numpy(),
               stin=ro.stin_all.cpu().numpy(), seq=ro.terrain_seq.copy(), nseq=ro.terrain_nseq.copy(), floor_z=ro.terrain_floor_z.copy())
    other = _ppo("jvrc_step")
    other.rollout.record_task_inputs = True
    other.sample_parallel_with_workers()
    r2 = other.rollout
    assert r2.last_mode == "resident"
    res = dict(obs=r2.obs.cpu().numpy(), act=r2.act.cpu().numpy(), rew=r2.rew.cpu().numpy(), done=r2.done.cpu().numpy(), tin=r2.tin_all.cpu().numpy(),
               stin=r2.stin_all.cpu().numpy())
    return algo.spec, algo.env.model, rec, res


def test_recording_rollout_is_the_resident_one_and_keeps_the_terrain_in_force():
    spec, model, rec, res = _stepping_record()
    for k, v in res.items():      # (of the two records, the columns include/lhw.h defines: nobody writes the pads of a [T][N][.] export)
        fields = dict(tin=_lib.TASK_INPUT_FIELDS, stin=_lib.STEP_TASK_INPUT_FIELDS).get(k)
        cols = slice(None) if fields is None else np.concatenate([np.arange(o, o + n) for o, n in fields.values()])
        assert np.array_equal(np.ascontiguousarray(rec[k][..., cols]).view(np.uint8), np.ascontiguousarray(v[..., cols]).view(np.uint8)), k
    S_ = _lib.STEP_TASK_INPUT_FIELDS
    T, N = rec["done"].shape
    assert T == 12 and N == 4 and rec["seq"].shape == (T, N, 20, 4) and (rec["nseq"] >= 1).all()
    checked = 0
    for t in range(T):
        for e in range(N):
            if t > 0 and rec["done"][t - 1, e]:
                continue
            t1 = int(rec["stin"][t, e, S_["t1"][0]])
            assert rec["nseq"][t, e] == int(rec["stin"][t, e, S_["nseq"][0]])
            assert np.array_equal(rec["seq"][t, e, t1], rec["stin"][t, e, S_["target1"][0]:S_["target1"][0] + 4]), (t, e)
            checked += 1
    assert checked >= T * N // 2


def test_frames_of_the_stepping_record_show_terrain_and_markers():
    spec, model, rec, _ = _stepping_record()
    box0, floor = spec.terrain_ids()
    hidden = list(range(box0, box0 + markers.NBOX)) + [floor]
    r = Renderer(model, 64, 48, device=0, hidden_geoms=hidden)
    q0 = _lib.TASK_INPUT_FIELDS["qpos"][0]
    fr, e = slice(0, 3), 0
    qpos = rec["tin"][fr, e, q0:q0 + model.nq]
    box_h = np.asarray(model.arrays["geom_size"]).reshape(-1, 3)[box0:box0 + markers.NBOX, 2]
    marks = markers.step_markers(rec["tin"][fr, e], rec["stin"][fr, e], rec["seq"][fr, e], rec["nseq"][fr, e], model, qpos, spec.body_ids()[2:4])
    terrain = markers.step_terrain(rec["seq"][fr, e], rec["nseq"][fr, e], rec["floor_z"][fr, e], box_h)
    dyn = markers.step_terrain(rec["seq"][fr, e], rec["nseq"][fr, e], rec["floor_z"][fr, e], box_h).merge(marks).arrays(3)
    G = r.n_geoms
    assert G + dyn["type"].shape[1] <= _lib.RENDER_SCENE_MAX_GEOMS and terrain.count(0) == 21
    rgb, hit, depth, layers, layer_hit = r.render(qpos, aux=True, markers=dyn)
    assert rgb.shape == (3, 48, 64, 3)
    ids = hit // 8
    assert ((ids >= G) & (ids < G + markers.NBOX)).any()                               # a terrain box
    sphere = [m for m in range(dyn["type"].shape[1]) if dyn["rgba"][0, m].tolist() == [1.0, 0.0, 0.0, 0.1]]
    assert len(sphere) == 1 and dyn["size"][0, sphere[0], 0] == markers.TARGET_RADIUS
    assert (layer_hit[0] // 8 == G + sphere[0]).any() and (layers > 0).any()             # the t1 target's translucent sphere
    bare = r.render(qpos, markers=marks)                                                 # the same markers with the terrain hidden
    assert not torch.equal(rgb, bare)


def test_frames_of_a_walking_record_show_the_velocity_arrows():
    algo = _ppo("jvrc_walk")
    algo.rollout.record_task_inputs = True
    algo.sample_parallel_with_workers()
    tin = algo.rollout.tin_all.cpu().numpy()
    F = _lib.TASK_INPUT_FIELDS
    forward = np.argwhere(tin[:, :, F["mode"][0]] == markers.MODE_FORWARD)
    if len(forward):
        rows = tin[forward[0][0]:forward[0][0] + 1, forward[0][1]]
    else:      # no env drew the mode in 12 steps: the test's own command on a recorded state
        rows = tin[5:6, 0].copy()
        rows[:, F["mode"][0]] = markers.MODE_FORWARD
        rows[:, F["mode_ref"][0]:F["mode_ref"][0] + 3] = (0.0, 0.4, 0.0)
    rows = rows.copy()
    rows[:, F["qvel"][0]:F["qvel"][0] + 2] += (0.3, 0.2)      # (a measured velocity that shows)
    model = algo.env.model
    r = Renderer(model, 64, 48, device=0)
    qpos = rows[:, F["qpos"][0]:F["qpos"][0] + model.nq]
    m = markers.walk_markers(rows)
    assert m.count(0) >= 2
    rgb, hit, depth, layers, layer_hit = r.render(qpos, aux=True, markers=m)
    plain = r.render(qpos, aux=True, markers=markers.Markers())
    assert torch.equal(hit, plain[1]) and not torch.equal(rgb, plain[0])                # translucent arrows: the opaque picture stays, the colours change
    assert (layer_hit // 8 >= r.n_geoms).any() and int(layers.max()) >= 1
