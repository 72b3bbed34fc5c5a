"""Forward kinematics of a compiled ``model.Model`` for any ``qpos`` (host-side, float64 numpy, vectorised over frames).

Generalises ``mjcf._kinematics0`` (body frames at ``qpos0``) to what ``mjcf.py`` compiles: a free root, hinge / slide chains and
welded bodies -- MuJoCo's ``mj_kinematics`` for that subset: a body starts from its parent's frame composed with its own offset, and
every joint of the body then moves it about the joint's anchor (hinge) or along its axis (slide); a free joint sets the frame from
``qpos`` outright, its quaternion normalised.  ``render.py`` poses the geoms of a recorded trajectory with it.
"""
from __future__ import annotations

import numpy as np

from .model import JNT_FREE, JNT_HINGE, JNT_SLIDE, Model


def _quat_mul(a, b):
    aw, ax, ay, az = (a[..., k] for k in range(4))
    bw, bx, by, bz = (b[..., k] for k in range(4))
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], axis=-1)


def _quat2mat(q):
    w, x, y, z = (q[..., k] for k in range(4))
    return np.stack([w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z], axis=-1).reshape(q.shape[:-1] + (3, 3))


def body_poses(model: Model, qpos):
    """(xpos [F][nbody][3], xquat [F][nbody][4], xmat [F][nbody][3][3]) of the body frames for qpos [F][nq]."""
    a = model.arrays
    q = np.atleast_2d(np.asarray(qpos, dtype=np.float64))
    if q.shape[1] != model.nq:
        raise ValueError(f"qpos has {q.shape[1]} columns, the model nq = {model.nq}")
    F, nb = q.shape[0], model.nbody
    xpos = np.zeros((F, nb, 3))
    xquat = np.zeros((F, nb, 4))
    xquat[:, :, 0] = 1.0
    xmat = np.tile(np.eye(3), (F, nb, 1, 1))
    qpos0 = np.asarray(a["qpos0"], dtype=np.float64)
    for b in range(1, nb):
        p = int(a["body_parentid"][b])
        j0, nj = int(a["body_jntadr"][b]), int(a["body_jntnum"][b])
        if nj == 1 and a["jnt_type"][j0] == JNT_FREE:
            adr = int(a["jnt_qposadr"][j0])
            pos = q[:, adr:adr + 3].copy()
            quat = q[:, adr + 3:adr + 7] / np.linalg.norm(q[:, adr + 3:adr + 7], axis=1, keepdims=True)
        else:
            pos = xpos[:, p] + np.einsum("fij,j->fi", xmat[:, p], a["body_pos"][b])
            quat = _quat_mul(xquat[:, p], np.broadcast_to(a["body_quat"][b], (F, 4)))
            for j in range(j0, j0 + nj):
                t, adr = int(a["jnt_type"][j]), int(a["jnt_qposadr"][j])
                R = _quat2mat(quat)
                dq = q[:, adr] - qpos0[adr]
                if t == JNT_SLIDE:
                    pos = pos + dq[:, None] * np.einsum("fij,j->fi", R, a["jnt_axis"][j])
                elif t == JNT_HINGE:
                    anchor = pos + np.einsum("fij,j->fi", R, a["jnt_pos"][j])
                    half = 0.5 * dq
                    qj = np.concatenate([np.cos(half)[:, None], np.sin(half)[:, None] * a["jnt_axis"][j][None, :]], axis=1)
                    quat = _quat_mul(quat, qj)
                    pos = anchor - np.einsum("fij,j->fi", _quat2mat(quat), a["jnt_pos"][j])
                else:
                    raise ValueError(f"joint {model.jnt_names[j]!r}: type {t} is not a free root, a hinge or a slide")
            quat = quat / np.linalg.norm(quat, axis=1, keepdims=True)
        xpos[:, b], xquat[:, b], xmat[:, b] = pos, quat, _quat2mat(quat)
    return xpos, xquat, xmat


def geom_poses(model: Model, qpos):
    """(pos [F][G][3], mat [F][G][9]) in float64: world position and row-major world rotation (columns = the geom's axes) of every
    geom of `model` for qpos [F][nq]."""
    a = model.arrays
    xpos, _, xmat = body_poses(model, qpos)
    gb = np.asarray(a["geom_bodyid"], dtype=np.int64)
    gmat = _quat2mat(np.asarray(a["geom_quat"], dtype=np.float64).reshape(-1, 4))
    pos = xpos[:, gb] + np.einsum("fgij,gj->fgi", xmat[:, gb], np.asarray(a["geom_pos"], dtype=np.float64).reshape(-1, 3))
    mat = np.einsum("fgij,gjk->fgik", xmat[:, gb], gmat)
    return pos, mat.reshape(mat.shape[0], mat.shape[1], 9)
