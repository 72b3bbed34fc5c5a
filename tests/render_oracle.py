"""TEST INFRASTRUCTURE: an independent numpy ray caster for the primitive geoms, the oracle of lhw_render_frames.

Written from the definitions in include/lhw.h, vectorised over the pixels of one image, in world coordinates with the camera at its
true position (no camera-relative trick, no tiles, no culling; the box is six face tests, not slabs).  It shares only the geom type
codes with the product.  float64 by default; `dtype=np.float32` evaluates the SAME formulas in float32, which is how the depth
tolerance below was measured.

Per pixel: rgb (uint8), hit (geom * 8 + part, -1 background), depth (ray parameter t, +inf background) and `stable`.  A pixel is stable
when (a) the tuple (hit, shadow flag, checker parity) is the same for the centre ray and for four rays offset by +-0.02 pixel in x and
in y (0.02 px is about 200 times the float32 direction error), and (b) the second-nearest surface along the centre ray lies more than
1e-3 (relative) behind the nearest.  The expected unstable share is 2 x 0.02 x (edge length in px) / area, about 0.5 % for the test
scenes; a scene must stay below MAX_UNSTABLE.

DEPTH_RTOL: measured, not chosen.  tests/render_checks.measure_depth_error() evaluates these formulas in float32 on every scene of the
render tests and takes the largest relative depth difference to float64 over the stable pixels: 5.5e-6, recorded as 5.6e-6 (the tilted
plane alone, at the pixels next to its horizon, where t = -o.z / d.z divides by a d.z of a few 1e-3; every other scene, the finite
primitives and the axis-aligned plane, stays below 3.5e-7).  DEPTH_RTOL = 8 x 5.6e-6 = 4.48e-5; the factor covers FMA contraction and
the different operation order of the kernel.  tests/test_render.py holds the constant to the measurement.
"""
import numpy as np

PLANE, SPHERE, CAPSULE, ELLIPSOID, CYLINDER, BOX = 0, 2, 3, 4, 5, 6
MAX_UNSTABLE = 0.03
MEASURED_F32_DEPTH_ERROR = 5.6e-6
DEPTH_RTOL = 8 * MEASURED_F32_DEPTH_ERROR
OFFSET_PX = 0.02
SECOND_SURFACE_REL = 1e-3

SETTINGS = dict(fovy_deg=45.0, light_dir=(0.3, -0.5, 1.0), ambient=0.35, diffuse=0.65, background=(0.55, 0.70, 0.90), checker_size=0.5,
                shadows=True)


def _dot(a, b):
    return (a * b).sum(axis=-1)


def _closest_approach_roots(o, d, r):
    """ray parameters where o + t d meets the sphere / circle of radius r around the origin (+inf: none)"""
    a = _dot(d, d)
    ok = a > 0
    a1 = np.where(ok, a, 1)
    tc = -_dot(o, d) / a1
    q = o + tc[:, None] * d
    h2 = r * r - _dot(q, q)
    ok &= h2 >= 0
    h = np.sqrt(np.where(ok, h2, 0) / a1)
    inf = np.array(np.inf, dtype=o.dtype)
    return np.where(ok, tc - h, inf), np.where(ok, tc + h, inf)


def _candidates(gtype, size, o, d):
    """every surface point of one geom along the rays o + t d (geom frame): list of (t [P] with +inf where there is none, part)"""
    dt = o.dtype
    inf = np.array(np.inf, dtype=dt)
    out = []
    if gtype == PLANE:
        nz = d[:, 2] != 0
        out.append((np.where(nz, -o[:, 2] / np.where(nz, d[:, 2], 1), inf), 0))
    elif gtype == SPHERE:
        out += [(t, 0) for t in _closest_approach_roots(o, d, size[0])]
    elif gtype == ELLIPSOID:
        out += [(t, 0) for t in _closest_approach_roots(o / size, d / size, dt.type(1))]
    elif gtype in (CAPSULE, CYLINDER):
        r, hl = size[0], size[1]
        for t in _closest_approach_roots(o[:, :2], d[:, :2], r):
            z = o[:, 2] + np.where(np.isfinite(t), t, 0) * d[:, 2]
            out.append((np.where(np.abs(z) <= hl, t, inf), 0))
        for e, ze in ((1, -hl), (2, hl)):
            if gtype == CAPSULE:
                oc = o - np.array([0, 0, ze], dtype=dt)
                for t in _closest_approach_roots(oc, d, r):
                    z = oc[:, 2] + np.where(np.isfinite(t), t, 0) * d[:, 2]
                    out.append((np.where(z < 0 if e == 1 else z > 0, t, inf), e))
            else:
                nz = d[:, 2] != 0
                t = np.where(nz, (ze - o[:, 2]) / np.where(nz, d[:, 2], 1), inf)
                tt = np.where(np.isfinite(t), t, 0)
                x, y = o[:, 0] + tt * d[:, 0], o[:, 1] + tt * d[:, 1]
                out.append((np.where(x * x + y * y <= r * r, t, inf), e))
    elif gtype == BOX:
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            nz = d[:, a] != 0
            for sign in (-1, 1):
                t = np.where(nz, (sign * size[a] - o[:, a]) / np.where(nz, d[:, a], 1), inf)
                tt = np.where(np.isfinite(t), t, 0)
                inside = (np.abs(o[:, b] + tt * d[:, b]) <= size[b]) & (np.abs(o[:, c] + tt * d[:, c]) <= size[c])
                out.append((np.where(inside, t, inf), 2 * a + (1 if sign > 0 else 0)))
    else:
        raise ValueError(f"geom type {gtype}")
    return [(np.where(t > 0, t, inf), part) for t, part in out]


def _normal(gtype, size, p, part, o):
    """outward unit normal (geom frame) at the surface points p [P][3] of parts `part` [P]; o: the ray origins (planes face them)"""
    n = np.zeros_like(p)
    if gtype == PLANE:
        n[:, 2] = np.where(o[:, 2] >= 0, 1, -1)
    elif gtype == SPHERE:
        n = p.copy()
    elif gtype == ELLIPSOID:
        n = p / (size * size)
    elif gtype == BOX:
        n[np.arange(len(p)), part // 2] = np.where(part % 2 == 1, 1, -1)
    else:
        body, lo, hi = part == 0, part == 1, part == 2
        n[:, :2] = np.where((body | (gtype == CAPSULE))[:, None], p[:, :2], 0)
        if gtype == CAPSULE:
            n[:, 2] = np.where(lo, p[:, 2] + size[1], np.where(hi, p[:, 2] - size[1], 0))
        else:
            n[:, 2] = np.where(lo, -1, np.where(hi, 1, 0))
    return n / np.maximum(np.sqrt(_dot(n, n)), np.finfo(p.dtype).tiny)[:, None]


def _nearest(scene, O, D, want_second=False):
    """nearest drawn surface along the rays (world): t, geom, part (and the second-nearest t)"""
    P = len(O)
    dt = O.dtype
    best = np.full(P, np.inf, dtype=dt)
    second = np.full(P, np.inf, dtype=dt)
    geom = np.full(P, -1, dtype=np.int64)
    part = np.zeros(P, dtype=np.int64)
    for g in range(len(scene["type"])):
        if scene["rgba"][g][3] == 0:
            continue
        R = scene["mat"][g].astype(dt)
        o, d = (O - scene["pos"][g].astype(dt)) @ R, D @ R
        for t, prt in _candidates(int(scene["type"][g]), scene["size"][g].astype(dt), o, d):
            closer = t < best
            second = np.where(closer, best, np.minimum(second, t))
            geom, part = np.where(closer, g, geom), np.where(closer, prt, part)
            best = np.where(closer, t, best)
    return (best, geom, part, second) if want_second else (best, geom, part)


def _trace(scene, cam_pos, cam_rows, W, H, st, dt, dx=0.0, dy=0.0):
    right, up, fwd = (np.asarray(cam_rows, dtype=np.float64).reshape(3, 3)[k].astype(dt) for k in range(3))
    tan_half = dt(np.tan(np.radians(st["fovy_deg"]) / 2))
    ys, xs = np.mgrid[0:H, 0:W]
    sx = (2 * (xs.reshape(-1).astype(dt) + dt(0.5 + dx)) / dt(W) - 1) * tan_half * dt(W / H)
    sy = -(2 * (ys.reshape(-1).astype(dt) + dt(0.5 + dy)) / dt(H) - 1) * tan_half
    D = fwd[None, :] + sx[:, None] * right[None, :] + sy[:, None] * up[None, :]
    D = D / np.sqrt(_dot(D, D))[:, None]
    O = np.broadcast_to(np.asarray(cam_pos, dtype=np.float64).astype(dt), D.shape)
    t, geom, part, second = _nearest(scene, O, D, want_second=True)
    hitm = geom >= 0
    tt = np.where(hitm, t, 0)
    Pw = O + tt[:, None] * D
    light = np.asarray(st["light_dir"], dtype=np.float64)
    light = (light / np.linalg.norm(light)).astype(dt)
    n = np.zeros_like(Pw)
    for g in np.unique(geom[hitm]):
        m = geom == g
        R = scene["mat"][g].astype(dt)
        pg = scene["pos"][g].astype(dt)
        nl = _normal(int(scene["type"][g]), scene["size"][g].astype(dt), (Pw[m] - pg) @ R, part[m], (O[m] - pg) @ R)
        n[m] = nl @ R.T
    ndl = np.maximum(_dot(n, light[None, :]), 0)
    shadow = np.zeros(len(D), dtype=bool)
    if st["shadows"]:
        m = hitm & (ndl > 0)
        ts, _, _ = _nearest(scene, Pw[m] + dt(1e-3) * n[m], np.broadcast_to(light, Pw[m].shape))
        shadow[m] = np.isfinite(ts)
    c = st["checker_size"]
    parity = np.zeros(len(D), dtype=np.int64)
    if c > 0:
        isplane = hitm & (np.asarray(scene["type"])[np.maximum(geom, 0)] == PLANE)
        parity = np.where(isplane, (np.floor(Pw[:, 0] / dt(c)) + np.floor(Pw[:, 1] / dt(c))).astype(np.int64) & 1, 0)
    rgb3 = np.asarray(scene["rgba"], dtype=np.float64)[np.maximum(geom, 0), :3].astype(dt)
    shade = dt(st["ambient"]) + dt(st["diffuse"]) * ndl * np.where(shadow, 0, 1).astype(dt)
    col = rgb3 * np.where(parity == 1, dt(0.8), dt(1))[:, None] * shade[:, None]
    col = np.where(hitm[:, None], col, np.asarray(st["background"], dtype=np.float64).astype(dt)[None, :])
    rgb = np.floor(255 * np.minimum(1, np.maximum(0, col)) + dt(0.5)).astype(np.uint8)
    hit = np.where(hitm, geom * 8 + part, -1)
    depth = np.where(hitm, t, np.inf)
    return dict(rgb=rgb.reshape(H, W, 3), hit=hit.reshape(H, W).astype(np.int32), depth=depth.reshape(H, W), shadow=shadow.reshape(H, W),
                parity=parity.reshape(H, W), second=second.reshape(H, W))


def render(scene, cam_pos, cam_rows, W, H, settings=None, dtype=np.float64, stable=True):
    """One image of `scene` = dict(type [G], size [G][3], rgba [G][4], pos [G][3], mat [G][3][3] world rotation) from the camera at
    cam_pos with rows (right, up, forward).  Returns dict(rgb, hit, depth, stable, shadow, parity)."""
    st = dict(SETTINGS, **(settings or {}))
    dt = np.dtype(dtype).type
    scene = {k: np.asarray(v) for k, v in scene.items()}
    scene["mat"] = scene["mat"].reshape(-1, 3, 3)
    r = _trace(scene, cam_pos, cam_rows, W, H, st, dt)
    if stable:
        ok = r["second"] > r["depth"] * (1 + SECOND_SURFACE_REL)
        ok |= r["hit"] < 0
        for dx, dy in ((OFFSET_PX, 0), (-OFFSET_PX, 0), (0, OFFSET_PX), (0, -OFFSET_PX)):
            o = _trace(scene, cam_pos, cam_rows, W, H, st, dt, dx, dy)
            ok &= (o["hit"] == r["hit"]) & (o["shadow"] == r["shadow"]) & (o["parity"] == r["parity"])
        r["stable"] = ok
    return r
