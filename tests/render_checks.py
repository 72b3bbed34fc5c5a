"""TEST INFRASTRUCTURE: the scenes of the render tests and the comparison with tests/render_oracle.py, shared by the emulated
(tests/test_render.py) and the GPU (tests/test_render_gpu.py) suites.  `make(type, size, rgba, W, H, **settings)` builds the product's
Renderer on the library under test."""
import functools
import math

import numpy as np

from tests import render_oracle as O


def rot(axis, angle):
    """rotation matrix about `axis` by `angle` radians (Rodrigues)"""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * K @ K


def z_to(v):
    """a rotation whose third column (the local z axis) is v / |v|"""
    z = np.asarray(v, dtype=np.float64)
    z = z / np.linalg.norm(z)
    x = np.cross([0.0, 0.0, 1.0] if abs(z[2]) < 0.9 else [1.0, 0.0, 0.0], z)
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z], axis=1)


def camera(lookat=(0.0, 0.0, 0.0), distance=3.0, azimuth=90.0, elevation=-20.0):
    """(position, rows right / up / forward): the tracking camera as include/lhw.h and render.TrackingCamera define it, restated"""
    az, el = math.radians(azimuth), math.radians(elevation)
    fwd = np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])
    right = np.cross(fwd, [0, 0, 1.0])
    right /= np.linalg.norm(right)
    return np.asarray(lookat, dtype=np.float64) - distance * fwd, np.concatenate([right, np.cross(right, fwd), fwd])


def scene_of(geoms):
    """geoms: list of (type, size, rgba, pos, mat)"""
    return dict(type=np.array([g[0] for g in geoms], dtype=np.int32), size=np.array([(list(g[1]) + [0, 0, 0])[:3] for g in geoms], dtype=np.float64),
                rgba=np.array([g[2] for g in geoms], dtype=np.float64), pos=np.array([g[3] for g in geoms], dtype=np.float64),
                mat=np.array([np.asarray(g[4], dtype=np.float64).reshape(3, 3) for g in geoms]))


GENERIC = rot((1.0, 2.0, 3.0), 0.7)
PRIMITIVES = {"plane": (O.PLANE, (0, 0, 0)), "sphere": (O.SPHERE, (0.5,)), "capsule": (O.CAPSULE, (0.25, 0.5)), "ellipsoid": (O.ELLIPSOID, (0.6, 0.35, 0.25)),
              "cylinder": (O.CYLINDER, (0.4, 0.4)), "box": (O.BOX, (0.5, 0.35, 0.25))}
RED, GREEN, BLUE, YELLOW, PURPLE, GREY, WHITE = ((0.9, 0.3, 0.25, 1), (0.3, 0.8, 0.35, 1), (0.3, 0.45, 0.9, 1), (0.9, 0.8, 0.3, 1), (0.7, 0.4, 0.85, 1),
                                                 (0.5, 0.5, 0.5, 1), (0.9, 0.9, 0.9, 1))


def _single(name, rotated):
    t, size = PRIMITIVES[name]
    if name == "plane":      # seen from 3 m at a shallow angle, so that the horizon -- and the background above it -- is in the picture
        mat = rot((0.26, 0.97, 0.0), 0.4) if rotated else np.eye(3)      # (tilted sideways: the horizon crosses the picture diagonally)
        return scene_of([(t, size, GREY, (0, 0, -0.5), mat)]), camera(distance=3.0, azimuth=75.0, elevation=-10.0)
    return scene_of([(t, size, RED, (0, 0, 0), GENERIC if rotated else np.eye(3))]), camera(distance=3.0, azimuth=75.0, elevation=-20.0)


def _seven():
    return [(O.PLANE, (0, 0, 0), GREY, (0, 0, 0), np.eye(3)),                                  # the checkered floor
            (O.PLANE, (0, 0, 0), WHITE, (0, 2.6, 0), z_to((0.1, -1.0, 0.15))),                 # a wall behind the others
            (O.SPHERE, (0.3,), RED, (-0.6, -0.5, 0.35), np.eye(3)),
            (O.CAPSULE, (0.15, 0.4), GREEN, (0.2, -0.3, 0.65), GENERIC),
            (O.ELLIPSOID, (0.5, 0.3, 0.2), BLUE, (0.7, 0.5, 0.3), rot((0, 0, 1.0), 0.4)),
            (O.CYLINDER, (0.25, 0.3), YELLOW, (-0.3, 0.6, 0.35), np.eye(3)),
            (O.BOX, (0.3, 0.25, 0.2), PURPLE, (0.9, -0.6, 0.25), rot((0, 0, 1.0), 0.5))]


def _seven_plus():      # a thin 1.5 m capsule and a large flat ellipsoid that cross many tile corners: a bounding sphere that is too small loses them
    return _seven() + [(O.CAPSULE, (0.03, 0.75), RED, (-0.1, -0.9, 0.9), z_to((1.0, 0.3, 0.6))),
                       (O.ELLIPSOID, (1.3, 0.9, 0.06), YELLOW, (0.2, 0.9, 1.25), rot((1.0, 0.2, 0.0), 0.3))]


def _grid64(n=64):
    return scene_of([(O.SPHERE, (0.12,), (0.2 + 0.1 * (g % 8), 0.9 - 0.1 * (g // 8 % 8), 0.5, 1), (0.45 * (g % 8 - 3.5) + (3.9 if g >= 64 else 0.0), 0.0, 0.45 * (g // 8 % 8 - 3.5)), np.eye(3))
                     for g in range(n)])


_SCENE_CAM = camera(lookat=(0.1, 0.0, 0.45), distance=4.0, azimuth=70.0, elevation=-25.0)
NO_CHECKER = dict(checker_size=0.0)


@functools.lru_cache(maxsize=None)
def case(name):
    """(scene, (cam_pos, cam_rows), W, H, settings) of a named test case"""
    if name.startswith("single_"):
        _, prim, how = name.split("_")
        sc, cam = _single(prim, how == "rot")
        return sc, cam, 32, 24, (NO_CHECKER if prim == "plane" else {})
    if name.startswith("odd_"):       # W x H = 37 x 21: no multiple of the tile
        sc, cam = _single(name.split("_")[1], True)
        return sc, cam, 37, 21, {}
    if name == "seven":
        return scene_of(_seven()), _SCENE_CAM, 64, 48, {}
    if name == "seven_plus":
        return scene_of(_seven_plus()), _SCENE_CAM, 64, 48, {}
    if name == "grid64":
        return _grid64(), camera(distance=5.0, azimuth=90.0, elevation=0.0), 64, 48, {}
    raise KeyError(name)


ALL_CASES = [f"single_{p}_{h}" for p in PRIMITIVES for h in ("axis", "rot")] + ["odd_box", "odd_capsule", "seven", "seven_plus", "grid64"]


@functools.lru_cache(maxsize=None)
def oracle(name):
    sc, (cp, cr), W, H, st = case(name)
    r = O.render(sc, cp, cr, W, H, st)
    for v in r.values():
        v.setflags(write=False)
    return r


def measure_depth_error(names=ALL_CASES):
    """the oracle's own formulas in float32 against float64: {case: (largest relative depth difference over stable pixels, unstable share)}"""
    out = {}
    for n in names:
        sc, (cp, cr), W, H, st = case(n)
        r64, r32 = oracle(n), O.render(sc, cp, cr, W, H, st, dtype=np.float32, stable=False)
        m = r64["stable"] & (r64["hit"] >= 0)
        assert (r32["hit"][m] == r64["hit"][m]).all(), n
        out[n] = (float(np.max(np.abs(r32["depth"][m].astype(np.float64) / r64["depth"][m] - 1.0))) if m.any() else 0.0, float(1.0 - r64["stable"].mean()))
    return out


def draw(make, name, out=None, **override):
    """the product's (rgb, hit, depth) numpy images of a case on the library behind `make`"""
    sc, (cp, cr), W, H, st = case(name)
    r = make(sc["type"], sc["size"], sc["rgba"], W, H, **dict(st, **override))
    rgb, hit, depth = r.render_geoms(sc["pos"][None], sc["mat"].reshape(1, -1, 9), cp[None], cr[None], aux=True, out=out)
    return rgb[0].cpu().numpy(), hit[0].cpu().numpy(), depth[0].cpu().numpy()


def check_against_oracle(make, name, images=None, min_cover=None):
    """hit equal, depth within DEPTH_RTOL, |rgb - oracle| <= 1 level on the oracle's stable pixels (at most MAX_UNSTABLE of the image are not)"""
    ref = oracle(name)
    rgb, hit, depth = draw(make, name) if images is None else images
    st = ref["stable"]
    unstable = 1.0 - st.mean()
    covered = float((ref["hit"] >= 0).mean())
    assert unstable <= O.MAX_UNSTABLE, (name, unstable)
    if min_cover is not None:      # the test cannot pass on an empty picture
        assert min_cover <= covered <= 1.0 - min_cover, (name, covered)
    bad = st & (hit != ref["hit"])
    assert not bad.any(), (name, "hit differs at", np.argwhere(bad)[:5].tolist(), hit[bad][:5], ref["hit"][bad][:5])
    m = st & (ref["hit"] >= 0)
    derr = float(np.max(np.abs(depth[m].astype(np.float64) / ref["depth"][m] - 1.0))) if m.any() else 0.0
    cerr = int(np.max(np.abs(rgb[st].astype(np.int32) - ref["rgb"][st].astype(np.int32)))) if st.any() else 0
    print(f"{name}: unstable {unstable:.4f} covered {covered:.3f} depth rel err {derr:.3e} (tol {O.DEPTH_RTOL:.1e}) rgb err {cerr}")
    assert np.isinf(depth[st & (ref["hit"] < 0)]).all(), name
    assert derr <= O.DEPTH_RTOL, (name, derr)
    assert cerr <= 1, (name, cerr)
    return rgb, hit, depth
