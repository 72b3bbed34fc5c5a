"""TEST INFRASTRUCTURE: the scenes of the lhw_render_scene tests and the comparison with tests/render_scene_oracle.py, shared by the
emulated (tests/test_render_scene.py) and the GPU (tests/test_render_scene_gpu.py) suites, as tests/render_checks.py is for
lhw_render_frames.  `make(type, size, rgba, W, H, **settings)` builds the product's Renderer of the STATIC geoms on the library under
test; the dynamic geoms go to its render_scene.

A case is a dict: static (type / size / rgba [G], pos [F][G][3], mat [F][G][9]; G may be 0), dynamic (type [F][M], size, rgba, pos, mat;
M may be 0), cams (one (position, rows) per frame), W, H, settings, cone (whether a cone is drawn)."""
import functools

import numpy as np

from tests import render_checks as C
from tests import render_scene_oracle as O

CONE_SIZE = (0.6, 0.7)


def _static(geoms, F=1):
    sc = C.scene_of(geoms) if geoms else dict(type=np.zeros(0, np.int32), size=np.zeros((0, 3)), rgba=np.zeros((0, 4)), pos=np.zeros((0, 3)), mat=np.zeros((0, 3, 3)))
    return dict(type=sc["type"], size=sc["size"], rgba=sc["rgba"], pos=np.repeat(sc["pos"][None], F, axis=0), mat=np.repeat(sc["mat"].reshape(1, -1, 9), F, axis=0))


def _dynamic(frames):
    """frames: per frame a list of (type, size, rgba, pos, mat); shorter frames are padded with alpha-0 spheres"""
    F, M = len(frames), max((len(f) for f in frames), default=0)
    d = dict(type=np.full((F, M), O.SPHERE, dtype=np.int32), size=np.ones((F, M, 3)), rgba=np.zeros((F, M, 4)), pos=np.zeros((F, M, 3)), mat=np.tile(np.eye(3).reshape(9), (F, M, 1)))
    for f, geoms in enumerate(frames):
        for m, (t, size, rgba, pos, mat) in enumerate(geoms):
            d["type"][f, m], d["size"][f, m], d["rgba"][f, m], d["pos"][f, m] = t, (list(size) + [0, 0, 0])[:3], rgba, pos
            d["mat"][f, m] = np.asarray(mat, dtype=np.float64).reshape(9)
    return d


def _case(static, dynamic, cams, W, H, settings=None, cone=False):
    return dict(static=static, dynamic=dynamic, cams=cams, W=W, H=H, settings=settings or {}, cone=cone)


def _toward(p, cam_pos, dist, side=0.0, right=None):
    """the point `dist` metres from p towards the camera (negative: away from it), `side` metres along the camera's right axis"""
    p = np.asarray(p, dtype=np.float64)
    v = cam_pos - p
    return p + dist * v / np.linalg.norm(v) + (side * np.asarray(right) if right is not None else 0.0)


def alpha(rgba, a):
    return tuple(rgba[:3]) + (a,)


def _layers_seven(swap=False):
    cp, cr = C._SCENE_CAM
    right = cr[:3]
    box, caps, ell = (np.array(g[3]) for g in (C._seven()[6], C._seven()[3], C._seven()[4]))
    pair = [(O.SPHERE, (0.18,), alpha(C.YELLOW, 0.3), _toward(caps, cp, 0.6, -0.07, right), np.eye(3)),
            (O.SPHERE, (0.18,), alpha(C.BLUE, 0.6), _toward(caps, cp, 1.0, 0.07, right), np.eye(3))]
    if swap:      # the same two layers in the other order along the ray: the spheres exchange colour and alpha
        pair = [pair[0][:2] + (pair[1][2],) + pair[0][3:], pair[1][:2] + (pair[0][2],) + pair[1][3:]]
    behind = _toward(ell, cp, -0.7)
    behind[2] = 0.3
    extra = [(O.SPHERE, (0.2,), alpha(C.GREEN, 0.5), _toward(box, cp, 0.7), np.eye(3))] + pair + [
        (O.BOX, (0.35, 0.04, 0.25), alpha(C.RED, 0.2), behind, C.rot((0, 0, 1.0), -0.35))]
    return C._seven() + extra


def _layers_ten():
    # ten translucent slabs stacked along the view (+y) in front of an opaque wall; the ids run from the farthest (7) to the nearest (16), so that
    # the two dropped layers are the first two of them
    geoms = [(O.PLANE, (0, 0, 0), C.WHITE, (0, 2.0, 0), C.z_to((0, -1.0, 0)))]
    geoms += [(O.SPHERE, (0.1,), C.RED, (0.9 * np.cos(k), 1.5, 0.9 * np.sin(k)), np.eye(3)) for k in range(6)]
    cols = [C.RED, C.GREEN, C.BLUE, C.YELLOW, C.PURPLE]
    # (eight of them fill the picture, the two nearest cover a part of it: eight layers there, ten candidates elsewhere, few edges at 32 x 24)
    geoms += [(O.BOX, (3.0, 0.02, 3.0) if i < 8 else (0.45, 0.02, 0.3), alpha(cols[i % 5], 0.1 + 0.02 * i), (0.1 * (i - 8), 1.0 - 0.2 * i, 0.05 * (i - 8)), np.eye(3)) for i in range(10)]
    return geoms


GRID_COLS, GRID_ROWS, GRID_PITCH, GRID_R = 13, 10, 0.4, 0.14


def grid_pos(k):
    """grid place k: row 0 is the TOP row"""
    return np.array([GRID_PITCH * (k % GRID_COLS - (GRID_COLS - 1) / 2), 0.0, GRID_PITCH * ((GRID_ROWS - 1) / 2 - k // GRID_COLS)])


GRID_SHADOWED, GRID_OCCLUDER = 5, 129


def _grid130():
    light = np.asarray(O.SETTINGS["light_dir"], dtype=np.float64)
    light /= np.linalg.norm(light)
    geoms = [(O.SPHERE, (GRID_R,), (0.2 + 0.06 * (g % GRID_COLS), 0.9 - 0.08 * (g // GRID_COLS), 0.5, 1), grid_pos(g), np.eye(3)) for g in range(129)]
    geoms.append((O.SPHERE, (GRID_R,), C.WHITE, grid_pos(GRID_SHADOWED) + 0.45 * light, np.eye(3)))      # id 129, between geom 5 and the light
    return geoms


@functools.lru_cache(maxsize=None)
def case(name):
    if name in ("single_cone_axis", "single_cone_rot", "odd_cone"):
        g = [(O.CONE, CONE_SIZE, C.RED, (0, 0, 0), np.eye(3) if name.endswith("axis") else C.z_to((0.7, 0.45, -0.55)))]      # (rotated: the base faces the camera)
        W, H = (37, 21) if name == "odd_cone" else (32, 24)
        return _case(_static([]), _dynamic([g]), [C.camera(distance=3.0, azimuth=75.0, elevation=-20.0)], W, H, cone=True)
    if name in ("arrow_end", "arrow_side"):
        from learninghumanoidwalking_amd.markers import Markers
        m = Markers().arrow(0, (0.0, -0.45, 0.0), (0.0, 1.0, 0.0), 0.12, 0.9, C.BLUE)
        cam = C.camera(lookat=(0, 0.05, 0), distance=2.0, azimuth=(-90.0 if name == "arrow_end" else 0.0), elevation=(-4.0 if name == "arrow_end" else -15.0))
        return _case(_static([]), m.arrays(1), [cam], 32, 24, cone=True)
    if name in ("layers_seven", "layers_seven_swapped"):
        g = _layers_seven(swap=name.endswith("swapped"))
        return _case(_static(g[:7]), _dynamic([g[7:]]), [C._SCENE_CAM], 64, 48)
    if name == "layers_ten":
        g = _layers_ten()
        return _case(_static(g[:7]), _dynamic([g[7:]]), [C.camera(lookat=(0, 0, 0), distance=3.0, azimuth=90.0, elevation=0.0)], 32, 24, C.NO_CHECKER)
    if name == "grid130":
        g = _grid130()
        return _case(_static(g[:100]), _dynamic([g[100:]]), [C.camera(distance=6.0, azimuth=90.0, elevation=0.0)], 64, 48)
    if name == "dynamic_three":      # a box that changes its height, a sphere that changes its colour, a cone marker that is absent in frame 1
        static = _static([(O.PLANE, (0, 0, 0), C.GREY, (0, 0, 0), np.eye(3)), (O.CAPSULE, (0.15, 0.3), C.GREEN, (0.6, 0.1, 0.5), C.GENERIC)], F=3)
        frames = []
        for f in range(3):
            h = 0.15 + 0.15 * f
            frames.append([(O.BOX, (0.3, 0.25, h), C.PURPLE, (-0.5, 0.2, h + 0.05), C.rot((0, 0, 1.0), 0.4)),
                           (O.SPHERE, (0.25,), (C.RED, C.YELLOW, alpha(C.BLUE, 0.5))[f], (0.1, -0.5, 0.3), np.eye(3)),
                           (O.CONE, (0.2, 0.25), alpha(C.WHITE, 0.0 if f == 1 else 1.0), (0.1, 0.6, 0.7), C.rot((1.0, 0, 0), 0.5))])
        cams = [C.camera(lookat=(0, 0, 0.35), distance=3.5, azimuth=70.0 + 10.0 * f, elevation=-25.0) for f in range(3)]
        return _case(static, _dynamic(frames), cams, 64, 48, dict(checker_size=2.0), cone=True)
    if name == "odd_layers":         # 37 x 21, a translucent sphere over the clipped tiles at the right and the bottom edge
        cam = C.camera(distance=3.0, azimuth=75.0, elevation=-20.0)
        far = _toward((0, 0, 0), cam[0], 0.8, 0.75, cam[1][:3]) - 0.45 * cam[1][3:6]
        return _case(_static([(O.BOX, (0.5, 0.35, 0.25), C.RED, (0, 0, 0), C.GENERIC)]),
                     _dynamic([[(O.SPHERE, (0.9,), alpha(C.BLUE, 0.4), far, np.eye(3)), (O.SPHERE, (0.3,), alpha(C.YELLOW, 0.7), (0.0, -0.7, 0.1), np.eye(3))]]), [cam], 37, 21)
    raise KeyError(name)


NO_CONE_CASES = ["layers_seven", "layers_seven_swapped", "layers_ten", "grid130", "odd_layers"]
CONE_CASES = ["single_cone_axis", "single_cone_rot", "odd_cone", "arrow_end", "arrow_side", "dynamic_three"]
ALL_CASES = NO_CONE_CASES + CONE_CASES


def frames_of(name):
    return len(case(name)["cams"])


@functools.lru_cache(maxsize=None)
def oracle(name, f=0):
    c = case(name)
    r = O.render(O.frame_scene(c["static"], c["dynamic"], f), c["cams"][f][0], c["cams"][f][1], c["W"], c["H"], c["settings"])
    for v in r.values():
        v.setflags(write=False)
    return r


def measure_depth_error(names=ALL_CASES):
    """the oracle's own formulas in float32 against float64: {case: (largest relative depth difference over stable pixels, largest unstable share)}"""
    out = {}
    for n in names:
        c = case(n)
        err, unst = 0.0, 0.0
        for f in range(frames_of(n)):
            r64 = oracle(n, f)
            r32 = O.render(O.frame_scene(c["static"], c["dynamic"], f), c["cams"][f][0], c["cams"][f][1], c["W"], c["H"], c["settings"], dtype=np.float32, stable=False)
            m = r64["stable"] & (r64["hit"] >= 0)
            assert (r32["hit"][m] == r64["hit"][m]).all(), n
            if m.any():
                err = max(err, float(np.max(np.abs(r32["depth"][m].astype(np.float64) / r64["depth"][m] - 1.0))))
            unst = max(unst, float(1.0 - r64["stable"].mean()))
        out[n] = (err, unst)
    return out


def draw(make, name, out=None, frames=None, **override):
    """the product's (rgb, hit, depth, layers, layer_hit) numpy images [F][...] of a case (frames: a slice of them) through lhw_render_scene"""
    c = case(name)
    sl = slice(None) if frames is None else frames
    r = make(c["static"]["type"], c["static"]["size"], c["static"]["rgba"], c["W"], c["H"], **dict(c["settings"], **override))
    cp, cr = np.stack([x[0] for x in c["cams"]])[sl], np.stack([x[1] for x in c["cams"]])[sl]
    res = r.render_scene(c["static"]["pos"][sl], c["static"]["mat"][sl], cp, cr, dynamic={k: v[sl] for k, v in c["dynamic"].items()}, aux=True, out=out)
    return tuple(x.cpu().numpy() for x in res)


def check_against_oracle(make, name, images=None, min_cover=None):
    """per frame: hit / layers / layer_hit equal, depth within the measured tolerance, |rgb - oracle| <= 1 level on the oracle's stable pixels
    (at most MAX_UNSTABLE of the image are not)"""
    images = draw(make, name) if images is None else images
    tol = O.DEPTH_RTOL
    for f in range(frames_of(name)):
        ref = oracle(name, f)
        rgb, hit, depth, layers, layer_hit = (x[f] for x in images)
        st = ref["stable"]
        unstable = 1.0 - st.mean()
        covered = float(((ref["hit"] >= 0) | (ref["layers"] > 0)).mean())
        assert unstable <= O.MAX_UNSTABLE, (name, f, unstable)
        if min_cover is not None:      # the test cannot pass on an empty picture
            assert min_cover <= covered <= 1.0 - min_cover, (name, f, covered)
        for key, img in (("hit", hit), ("layers", layers), ("layer_hit", layer_hit)):
            bad = st & (img != ref[key])
            assert not bad.any(), (name, f, key, "differs at", np.argwhere(bad)[:5].tolist(), img[bad][:5], ref[key][bad][:5])
        m = st & (ref["hit"] >= 0)
        derr = float(np.max(np.abs(depth[m].astype(np.float64) / ref["depth"][m] - 1.0))) if m.any() else 0.0
        cerr = int(np.max(np.abs(rgb[st].astype(np.int32) - ref["rgb"][st].astype(np.int32)))) if st.any() else 0
        print(f"{name}[{f}]: unstable {unstable:.4f} covered {covered:.3f} depth rel err {derr:.3e} (tol {tol:.1e}) rgb err {cerr} most layers {int(ref['layers'].max())}")
        assert np.isinf(depth[st & (ref["hit"] < 0)]).all(), (name, f)
        assert derr <= tol, (name, f, derr)
        assert cerr <= 1, (name, f, cerr)
    return images
