"""TEST INFRASTRUCTURE: an independent numpy ray caster for lhw_render_scene -- the oracle of tests/render_oracle.py extended by what
include/lhw.h adds for the scene entry: the cone, translucent layers with their compositing, and per-frame (dynamic) geoms.

Written from the definitions in include/lhw.h, in world coordinates with the camera at its true position, vectorised over the pixels of
one image.  It takes the candidates and normals of the old primitives from tests/render_oracle.py and shares only the type codes with
the product.  A frame of a scene with dynamic geoms is the concatenation of the static geoms and that frame's dynamic ones
(`frame_scene`).  float64 by default; `dtype=np.float32` evaluates the SAME formulas in float32 (the depth tolerance's measurement).

The cone is the union of explicit candidates: the two lateral roots and the base disc.  With z measured from the apex the lateral
surface is q(v) = x^2 + y^2 - k^2 z^2 = 0, k = r / (2 hl); the roots are tc +- sqrt(-q(p_c) / q(d)) with tc = -B(o, d) / q(d) the ray
parameter at which q is stationary and p_c the ray's point there -- for a thin cone far away p_c lies next to the axis, so that q(p_c) is
a difference of terms of the size of r^2, where b^2 - a c would be one of terms of the size of the distance squared.

Per pixel: rgb, hit / depth of the nearest OPAQUE surface, layers (the number of composited translucent layers), layer_hit (id * 8 +
part of the front-most layer, -1), layer_list [8] (id * 8 + part of every composited layer, front to back, -1 behind them), shadow,
parity and `stable`.  A pixel is stable when all three hold: (a) the tuple (opaque hit, shadow flag, checker parity, ordered list of
layer ids and parts) is the same for the centre ray and for the four rays offset by +-0.02 px; (b) every two consecutive surfaces
along the centre ray, of any drawn geom, up to the opaque one and the first behind it, lie more than 1e-3 (relative) apart; (c) where
more than eight layers lie in front of the opaque surface, the ninth lies more than 1e-3 (relative) behind the eighth.

DEPTH_RTOL: measured, not chosen -- the method of tests/render_oracle.py.  render_scene_checks.measure_depth_error() evaluates these
formulas in float32 on every scene of the scene tests and takes the largest relative depth difference to float64 over the stable pixels:
7.8e-7, recorded as 7.9e-7 (the rotated cone's base disc; the scenes without a cone stay below 3.4e-7).  That is below the 5.6e-6 of the
first oracle's scenes -- none of these has a plane seen next to its horizon -- so the cone needs no constant of its own.  DEPTH_RTOL = 8 x
7.9e-7 = 6.32e-6, the project's factor for FMA contraction and operation order.  tests/test_render_scene.py holds the constant to the
measurement.
"""
import numpy as np

from tests.render_oracle import BOX, CAPSULE, CYLINDER, ELLIPSOID, MAX_UNSTABLE, OFFSET_PX, PLANE, SECOND_SURFACE_REL, SETTINGS, SPHERE, _candidates, _dot, _normal

CONE = 32
MAX_LAYERS = 8
MAX_GEOMS = 256
MEASURED_F32_DEPTH_ERROR = 7.9e-7
DEPTH_RTOL = 8 * MEASURED_F32_DEPTH_ERROR


def _cone_candidates(size, o, d):
    dt = o.dtype
    inf = np.array(np.inf, dtype=dt)
    r, hl = size[0], size[1]
    k2 = (r / (2 * hl)) ** 2
    oa = o - np.array([0, 0, hl], dtype=dt)
    q = lambda u, v: u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1] - k2 * u[:, 2] * v[:, 2]
    a, b, c = q(d, d), q(oa, d), q(oa, oa)
    quad = a != 0
    a1 = np.where(quad, a, 1)
    tc = -b / a1
    pc = oa + tc[:, None] * d
    h2 = -q(pc, pc) / a1
    ok = quad & (h2 >= 0)
    h = np.sqrt(np.where(ok, h2, 0))
    lin = ~quad & (b != 0)
    roots = [np.where(ok, tc - h, inf), np.where(ok, tc + h, np.where(lin, -c / np.where(lin, 2 * b, 1), inf))]
    out = []
    for t in roots:
        z = oa[:, 2] + np.where(np.isfinite(t), t, 0) * d[:, 2]
        out.append((np.where((z <= 0) & (z >= -2 * hl), t, inf), 0))
    nz = d[:, 2] != 0
    t = np.where(nz, (-hl - o[:, 2]) / np.where(nz, d[:, 2], 1), inf)
    tt = np.where(np.isfinite(t), t, 0)
    x, y = o[:, 0] + tt * d[:, 0], o[:, 1] + tt * d[:, 1]
    out.append((np.where(x * x + y * y <= r * r, t, inf), 1))
    return [(np.where(t > 0, t, inf), part) for t, part in out]


def candidates(gtype, size, o, d):
    return _cone_candidates(size, o, d) if gtype == CONE else _candidates(gtype, size, o, d)


def normal(gtype, size, p, part, o):
    if gtype != CONE:
        return _normal(gtype, size, p, part, o)
    rho = np.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2)
    n = np.stack([p[:, 0], p[:, 1], rho * size[0] / (2 * size[1])], axis=1)
    n = np.where((part == 1)[:, None], np.array([0, 0, -1], dtype=p.dtype), n)
    l = np.sqrt(_dot(n, n))
    return np.where((l > 0)[:, None], n / np.where(l > 0, l, 1)[:, None], np.array([0, 0, 1], dtype=p.dtype))


def frame_scene(static, dynamic, f):
    """the geoms of frame f: the static ones (a dict of [G] arrays with per-frame pos / mat [F][G]) followed by the frame's dynamic ones"""
    parts = []
    if static is not None and len(static["type"]):
        parts.append(dict(type=static["type"], size=static["size"], rgba=static["rgba"], pos=np.asarray(static["pos"])[f], mat=np.asarray(static["mat"])[f].reshape(-1, 3, 3)))
    if dynamic is not None and np.asarray(dynamic["type"]).shape[1]:
        parts.append({k: (np.asarray(dynamic[k])[f].reshape(-1, 3, 3) if k == "mat" else np.asarray(dynamic[k])[f]) for k in ("type", "size", "rgba", "pos", "mat")})
    return {k: np.concatenate([np.asarray(p[k], dtype=np.int32 if k == "type" else np.float64) for p in parts]) for k in ("type", "size", "rgba", "pos", "mat")}


def _is_translucent(alpha):
    return (alpha > 0) & (alpha < 1)


def _local(scene, g, O, D, dt):
    R = scene["mat"][g].astype(dt)
    return (O - scene["pos"][g].astype(dt)) @ R, D @ R


def _nearest_opaque(scene, O, D):
    best = np.full(len(O), np.inf, dtype=O.dtype)
    for g in range(len(scene["type"])):
        al = scene["rgba"][g][3]
        if al == 0 or _is_translucent(al):
            continue
        o, d = _local(scene, g, O, D, O.dtype.type)
        for t, _ in candidates(int(scene["type"][g]), scene["size"][g].astype(O.dtype), o, d):
            best = np.minimum(best, t)
    return best


def _shade_inputs(scene, g, m, O, D, t, part, light, dt):
    """(n.l clipped at 0, world normal) at the points O + t D of geom g for the pixels m"""
    R = scene["mat"][g].astype(dt)
    pg = scene["pos"][g].astype(dt)
    Pw = O[m] + t[m][:, None] * D[m]
    n = normal(int(scene["type"][g]), scene["size"][g].astype(dt), (Pw - pg) @ R, part[m], (O[m] - pg) @ R) @ R.T
    return np.maximum(_dot(n, light[None, :]), 0), n, Pw


def _trace(scene, cam_pos, cam_rows, W, H, st, dt, dx=0.0, dy=0.0):
    right, up, fwd = (np.asarray(cam_rows, dtype=np.float64).reshape(3, 3)[k].astype(dt) for k in range(3))
    tan_half = dt(np.tan(np.radians(st["fovy_deg"]) / 2))
    ys, xs = np.mgrid[0:H, 0:W]
    sx = (2 * (xs.reshape(-1).astype(dt) + dt(0.5 + dx)) / dt(W) - 1) * tan_half * dt(W / H)
    sy = -(2 * (ys.reshape(-1).astype(dt) + dt(0.5 + dy)) / dt(H) - 1) * tan_half
    D = fwd[None, :] + sx[:, None] * right[None, :] + sy[:, None] * up[None, :]
    D = D / np.sqrt(_dot(D, D))[:, None]
    P = len(D)
    O = np.broadcast_to(np.asarray(cam_pos, dtype=np.float64).astype(dt), D.shape)
    inf = np.array(np.inf, dtype=dt)
    best, geom, part = np.full(P, np.inf, dtype=dt), np.full(P, -1, dtype=np.int64), np.zeros(P, dtype=np.int64)
    surfaces, tr = [], []      # every surface point's t; per translucent geom (id, nearest t, its part)
    types = np.asarray(scene["type"])
    for g in range(len(types)):
        al = scene["rgba"][g][3]
        if al == 0:
            continue
        o, d = _local(scene, g, O, D, dt)
        cands = candidates(int(types[g]), scene["size"][g].astype(dt), o, d)
        surfaces += [t for t, _ in cands]
        tg, pg = np.full(P, np.inf, dtype=dt), np.zeros(P, dtype=np.int64)
        for t, prt in cands:
            closer = t < tg
            tg, pg = np.where(closer, t, tg), np.where(closer, prt, pg)
        if _is_translucent(al):
            tr.append((g, tg, pg))
        else:
            closer = tg < best
            best, geom, part = np.where(closer, tg, best), np.where(closer, g, geom), np.where(closer, pg, part)
    hitm = geom >= 0
    light = np.asarray(st["light_dir"], dtype=np.float64)
    light = (light / np.linalg.norm(light)).astype(dt)
    c = st["checker_size"]
    bg = np.asarray(st["background"], dtype=np.float64).astype(dt)
    rgba = np.asarray(scene["rgba"], dtype=np.float64)

    def checker(Pw):
        return ((np.floor(Pw[:, 0] / dt(c)) + np.floor(Pw[:, 1] / dt(c))).astype(np.int64) & 1) if c > 0 else np.zeros(len(Pw), dtype=np.int64)

    # ---- the opaque surface
    ndl, n, Pw = np.zeros(P, dtype=dt), np.zeros((P, 3), dtype=dt), np.zeros((P, 3), dtype=dt)
    parity = np.zeros(P, dtype=np.int64)
    tt = np.where(hitm, best, 0)
    for g in np.unique(geom[hitm]):
        m = geom == g
        ndl[m], n[m], Pw[m] = _shade_inputs(scene, g, m, O, D, tt, part, light, dt)
        if types[g] == PLANE:
            parity[m] = checker(Pw[m])
    shadow = np.zeros(P, dtype=bool)
    if st["shadows"]:
        m = hitm & (ndl > 0)
        shadow[m] = np.isfinite(_nearest_opaque(scene, Pw[m] + dt(1e-3) * n[m], np.broadcast_to(light, Pw[m].shape)))
    shade = dt(st["ambient"]) + dt(st["diffuse"]) * ndl * np.where(shadow, 0, 1).astype(dt)
    col = rgba[np.maximum(geom, 0), :3].astype(dt) * np.where(parity == 1, dt(0.8), dt(1))[:, None] * shade[:, None]
    col = np.where(hitm[:, None], col, bg[None, :])

    # ---- the layers in front of it
    layer_list = np.full((MAX_LAYERS, P), -1, dtype=np.int64)
    nlay, ninfront = np.zeros(P, dtype=np.int64), np.zeros(P, dtype=np.int64)
    t8 = t9 = np.full(P, np.inf, dtype=dt)
    layer_parity = np.zeros((MAX_LAYERS, P), dtype=np.int64)
    if tr:
        T = np.stack([np.where(tg < best, tg, inf) for _, tg, _ in tr])                # (strictly in front of the opaque surface)
        order = np.argsort(T, axis=0, kind="stable")                                  # equal t: the lower geom id in front
        Ts = np.take_along_axis(T, order, axis=0)
        ninfront = np.isfinite(T).sum(axis=0)
        nlay = np.minimum(ninfront, MAX_LAYERS)
        if len(tr) > MAX_LAYERS:
            t8, t9 = Ts[MAX_LAYERS - 1], Ts[MAX_LAYERS]
        through, acc = np.ones(P, dtype=dt), np.zeros((P, 3), dtype=dt)
        for k in range(min(MAX_LAYERS, len(tr))):
            live = k < nlay
            for j, (g, tg, pg) in enumerate(tr):
                m = live & (order[k] == j)
                if not m.any():
                    continue
                layer_list[k, m] = g * 8 + pg[m]
                l_ndl, _, l_Pw = _shade_inputs(scene, g, m, O, D, np.where(np.isfinite(tg), tg, 0), pg, light, dt)
                lc = np.broadcast_to(rgba[g, :3].astype(dt), (int(m.sum()), 3))
                if types[g] == PLANE:
                    layer_parity[k, m] = checker(l_Pw)
                    lc = lc * np.where(layer_parity[k, m] == 1, dt(0.8), dt(1))[:, None]
                al = dt(rgba[g, 3])
                w = through[m] * al * (dt(st["ambient"]) + dt(st["diffuse"]) * l_ndl)
                acc[m] = acc[m] + w[:, None] * lc
                through[m] = through[m] * (dt(1) - al)
        col = np.where((nlay > 0)[:, None], acc + through[:, None] * col, col)
    rgb = np.floor(255 * np.minimum(1, np.maximum(0, col)) + dt(0.5)).astype(np.uint8)

    # ---- the smallest relative gap between consecutive surfaces up to the opaque one and the first behind it
    gap = np.full(P, np.inf)
    if surfaces:
        S = np.sort(np.stack(surfaces).astype(np.float64), axis=0)
        for i in range(len(S) - 1):
            both = np.isfinite(S[i]) & np.isfinite(S[i + 1]) & (S[i] <= best)
            gap = np.where(both, np.minimum(gap, S[i + 1] / np.where(both, S[i], 1) - 1), gap)
    im = lambda x: x.reshape(H, W)
    return dict(rgb=rgb.reshape(H, W, 3), hit=im(np.where(hitm, geom * 8 + part, -1)).astype(np.int32), depth=im(np.where(hitm, best, np.inf)),
                shadow=im(shadow), parity=im(parity), layers=im(nlay).astype(np.int32), layer_hit=im(layer_list[0]).astype(np.int32),
                layer_list=layer_list.reshape(MAX_LAYERS, H, W), layer_parity=layer_parity.reshape(MAX_LAYERS, H, W), in_front=im(ninfront), gap=im(gap),
                cut=im(np.where(np.isfinite(t9), t9 / np.where(np.isfinite(t8), t8, 1) - 1, np.inf)))


def render(scene, cam_pos, cam_rows, W, H, settings=None, dtype=np.float64, stable=True):
    """One image of `scene` = dict(type [G], size [G][3], rgba [G][4], pos [G][3], mat [G][3][3]) (frame_scene builds one from static and
    dynamic geoms) from the camera at cam_pos with rows (right, up, forward)."""
    st = dict(SETTINGS, **(settings or {}))
    dt = np.dtype(dtype).type
    scene = {k: np.asarray(v) for k, v in scene.items()}
    scene["mat"] = scene["mat"].reshape(-1, 3, 3)
    assert len(scene["type"]) <= MAX_GEOMS
    r = _trace(scene, cam_pos, cam_rows, W, H, st, dt)
    if stable:
        ok = (r["gap"] > SECOND_SURFACE_REL) & (r["cut"] > SECOND_SURFACE_REL)
        for dx, dy in ((OFFSET_PX, 0), (-OFFSET_PX, 0), (0, OFFSET_PX), (0, -OFFSET_PX)):
            o = _trace(scene, cam_pos, cam_rows, W, H, st, dt, dx, dy)
            ok &= (o["hit"] == r["hit"]) & (o["shadow"] == r["shadow"]) & (o["parity"] == r["parity"])
            ok &= (o["layer_list"] == r["layer_list"]).all(axis=0) & (o["layer_parity"] == r["layer_parity"]).all(axis=0)
        r["stable"] = ok
    return r
