"""Per-frame geoms for lhw_render_scene (include/lhw.h): the task markers and the stepping terrain of the reference's eval.

Every task of the reference has a draw_markers: the walking tasks an arrow of the commanded and one of the measured velocity above the
head (envs/jvrc/jvrc_walk.py:69-118, envs/h1/h1_walk.py:149-174), the stepping task its footstep sequence, the two current targets, the
foot frames and the origin (envs/jvrc/jvrc_step.py:78-198); the stepping task also places its terrain boxes at every reset
(tasks/stepping_task.py:320-334).  Here they are lists of primitive geoms per frame, built on the host in float64 from the task-input
records of a rollout, which `Renderer.render(..., markers=...)` draws behind the model's own geoms (ids G + m).
"""
from __future__ import annotations

import math

import numpy as np

from . import _lib

PLANE, SPHERE, CAPSULE, ELLIPSOID, CYLINDER, BOX, CONE = 0, 2, 3, 4, 5, 6, _lib.RENDER_CONE
MODE_STANDING, MODE_INPLACE, MODE_FORWARD = 0, 1, 2      # LHW_TIN_MODE of the walking tasks' record (csrc/lhw_humanoid_dev.h)
TARGET_RADIUS = 0.2                                      # tasks/stepping_task.py: target_radius
NBOX = 20

_CYAN, _RED, _BLUE, _GREY, _WHITE = (0, 1, 1, 1), (1, 0, 0, 1), (0, 0, 1, 1), (0.5, 0.5, 0.5, 1), (1, 1, 1, 1)


def z_to(v):
    """a rotation (3 x 3, columns = local axes) whose local z axis is v / |v|"""
    z = np.asarray(v, dtype=np.float64)
    z = z / np.linalg.norm(z)
    x = np.cross([0.0, 0.0, 1.0] if abs(z[2]) < 0.9 else [1.0, 0.0, 0.0], z)
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z], axis=1)


def yaw_mat(theta):
    c, s = math.cos(theta), math.sin(theta)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def quat_yaw(q):
    """the yaw of the z-y-x Euler angles of a unit quaternion (w, x, y, z): transforms3d's quat2euler(q)[2], which the reference uses"""
    w, x, y, z = (float(v) for v in q)
    return math.atan2(2.0 * (w * z + x * y), 1.0 - 2.0 * (y * y + z * z))


class Markers:
    """Lists of geoms per frame.  `arrays(F)` pads every frame to the longest list with alpha-0 geoms ("absent in this frame")."""

    def __init__(self):
        self._frames: dict[int, list] = {}

    def add(self, frame, type, size, rgba, pos, mat=None):
        """one geom in frame `frame`: size as geom_size (up to 3 values), rgba, world position, world rotation (3 x 3 or 9, default identity)"""
        size = (list(np.asarray(size, dtype=np.float64).reshape(-1)) + [0.0, 0.0, 0.0])[:3]
        mat = np.eye(3) if mat is None else np.asarray(mat, dtype=np.float64).reshape(3, 3)
        self._frames.setdefault(int(frame), []).append((int(type), size, [float(c) for c in rgba], np.asarray(pos, dtype=np.float64).reshape(3), mat))
        return self

    def arrow(self, frame, pos, axis_or_mat, radius, length, rgba):
        """An arrow from `pos` along the local z axis of `axis_or_mat` (a direction, or a rotation whose third column is one); a negative
        length points the other way, zero length draws nothing.  The head is a cone of base radius 2 * radius and height h = min(|L|, 4 *
        radius), the shaft a cylinder of `radius` over the remaining |L| - h, left out where that is <= 0.  These are OUR proportions:
        MuJoCo's own arrow (mjGEOM_ARROW) proportions are not known here, and no pixel parity with its renderer is claimed."""
        a = np.asarray(axis_or_mat, dtype=np.float64)
        L = float(length)
        if L == 0.0:
            return self
        R = a.reshape(3, 3) if a.size == 9 else z_to(a)
        if L < 0.0:
            R = R @ np.diag([1.0, -1.0, -1.0])      # half a turn about local x: local z points back
        L = abs(L)
        z = R[:, 2]
        pos = np.asarray(pos, dtype=np.float64).reshape(3)
        h = min(L, 4.0 * radius)
        if L - h > 0.0:
            self.add(frame, CYLINDER, (radius, 0.5 * (L - h)), rgba, pos + 0.5 * (L - h) * z, R)
        return self.add(frame, CONE, (2.0 * radius, 0.5 * h), rgba, pos + (L - 0.5 * h) * z, R)

    def merge(self, other):
        """append another builder's geoms, frame by frame, behind this one's"""
        for f, geoms in other._frames.items():
            self._frames.setdefault(f, []).extend(geoms)
        return self

    def count(self, frame) -> int:
        return len(self._frames.get(int(frame), ()))

    def arrays(self, F=None, M=None):
        """dict(type [F][M] int32, size [F][M][3], rgba [F][M][4], pos [F][M][3] world, mat [F][M][9]) in float64, the frames padded to M
        geoms (default: the longest list) by spheres of alpha 0"""
        F = (max(self._frames) + 1 if self._frames else 0) if F is None else int(F)
        if self._frames and (min(self._frames) < 0 or max(self._frames) >= F):
            raise ValueError(f"markers in frames {min(self._frames)}..{max(self._frames)}, but there are {F} frames")
        longest = max((len(g) for g in self._frames.values()), default=0)
        M = longest if M is None else int(M)
        if M < longest:
            raise ValueError(f"a frame holds {longest} markers, more than M = {M}")
        out = dict(type=np.full((F, M), SPHERE, dtype=np.int32), size=np.ones((F, M, 3)), rgba=np.zeros((F, M, 4)), pos=np.zeros((F, M, 3)),
                   mat=np.tile(np.eye(3).reshape(9), (F, M, 1)))
        for f, geoms in self._frames.items():
            for m, (t, size, rgba, pos, mat) in enumerate(geoms):
                out["type"][f, m], out["size"][f, m], out["rgba"][f, m], out["pos"][f, m], out["mat"][f, m] = t, size, rgba, pos, mat.reshape(9)
        return out


def walk_markers(task_inputs) -> Markers:
    """The walking tasks' arrows (jvrc_walk, h1_walk) from the LhwTaskInput records task_inputs [F][176] of one env, one frame per record:
    above the head, at head + (0, 0, 0.3), a blue arrow (0, 0, 1, 0.5) for the command and a green one (0, 1, 0, 0.5) for the measurement,
    radius 0.05, length 2 x the size value (the reference's size[2]).  FORWARD: the command along the root's heading (the yaw of qpos[3:7]),
    size value |mode_ref[1:3]|; the measurement along atan2(v_y, v_x) of qvel[0:2], size value the planar speed.  INPLACE: both vertical,
    size values mode_ref[0] and qvel[5] (negative: pointing down).  STANDING: none."""
    rec = np.atleast_2d(np.asarray(task_inputs, dtype=np.float64))
    F = _lib.TASK_INPUT_FIELDS
    cut = lambda row, k: row[F[k][0]:F[k][0] + F[k][1]]
    m = Markers()
    for f, row in enumerate(rec):
        mode, ref, q, v = int(round(row[F["mode"][0]])), cut(row, "mode_ref"), cut(row, "qpos"), cut(row, "qvel")
        at = cut(row, "head_xpos") + [0.0, 0.0, 0.3]
        if mode == MODE_FORWARD:
            yaw, vyaw = quat_yaw(q[3:7]), math.atan2(v[1], v[0])
            m.arrow(f, at, (math.cos(yaw), math.sin(yaw), 0.0), 0.05, 2.0 * float(np.hypot(ref[1], ref[2])), (0, 0, 1, 0.5))
            m.arrow(f, at, (math.cos(vyaw), math.sin(vyaw), 0.0), 0.05, 2.0 * float(np.hypot(v[0], v[1])), (0, 1, 0, 0.5))
        elif mode == MODE_INPLACE:
            m.arrow(f, at, np.eye(3), 0.05, 2.0 * float(ref[0]), (0, 0, 1, 0.5))
            m.arrow(f, at, np.eye(3), 0.05, 2.0 * float(v[5]), (0, 1, 0, 0.5))
    return m


def _target(m, f, step, rgba):
    m.add(f, SPHERE, (0.05,), rgba, step[:3])
    m.arrow(f, step[:3], (math.cos(step[3]), math.sin(step[3]), 0.0), 0.02, 0.5, rgba)


def step_markers(task_inputs, step_task_inputs, seq, nseq, model, qpos, foot_bodies=("R_ANKLE_P_S", "L_ANKLE_P_S")) -> Markers:
    """The stepping task's markers (envs/jvrc/jvrc_step.py:78-198) for F frames of one env: task_inputs [F][176] and step_task_inputs
    [F][32] are the two records, seq [F][20][>=4] (x y z theta) / nseq [F] the footstep sequence in force, qpos [F][nq] the poses and
    foot_bodies the (right, left) foot bodies of `model`, names or ids (default: the JVRC stand-in's, envs/jvrc_walk.py task_bodies).

    Every sequence step other than the targets t1 / t2: a cyan sphere (r 0.05) and an arrow (radius 0.02, length 0.5) along its theta;
    t1 in red and t2 in blue likewise, each inside a sphere of target_radius 0.2 with alpha 0.1; the two feet: a grey sphere and arrow at the
    record's force-site positions, pointing along the foot body's x axis (kinematics.body_poses); the origin: a white sphere and three
    axes of length 2, radius 0.01, alpha 0.2 (x red, y green, z blue).  Left out: the reference's "observed goal" markers, which it
    draws at root-frame coordinates as if they were world coordinates."""
    from .kinematics import body_poses
    stin = np.atleast_2d(np.asarray(step_task_inputs, dtype=np.float64))      # (task_inputs: the first record of the same steps; nothing of it is drawn yet)
    seq, nseq = np.asarray(seq, dtype=np.float64), np.asarray(nseq).reshape(-1).astype(int)
    S = _lib.STEP_TASK_INPUT_FIELDS
    xmat = body_poses(model, np.atleast_2d(np.asarray(qpos, dtype=np.float64)))[2]
    foot_bodies = [model.body_id(b) if isinstance(b, str) else int(b) for b in foot_bodies]
    m = Markers()
    for f in range(len(stin)):
        t1, t2 = int(round(stin[f, S["t1"][0]])), int(round(stin[f, S["t2"][0]]))
        for i in range(nseq[f]):
            if i not in (t1, t2):
                _target(m, f, seq[f, i], _CYAN)
        for t, rgba in ((t1, _RED), (t2, _BLUE)):
            if 0 <= t < nseq[f]:
                _target(m, f, seq[f, t], rgba)
                m.add(f, SPHERE, (TARGET_RADIUS,), rgba[:3] + (0.1,), seq[f, t, :3])
        for key, body in (("rsite_xpos", foot_bodies[0]), ("lsite_xpos", foot_bodies[1])):
            at = stin[f, S[key][0]:S[key][0] + 3]
            m.add(f, SPHERE, (0.05,), _GREY, at)
            m.arrow(f, at, xmat[f, body][:, 0], 0.02, 0.5, _GREY)
        m.add(f, SPHERE, (0.05,), _WHITE, (0, 0, 0))
        for axis, rgba in (((0, 0, 1.0), (0, 0, 1, 0.2)), ((1.0, 0, 0), (1, 0, 0, 0.2)), ((0, 1.0, 0), (0, 1, 0, 0.2))):
            m.arrow(f, (0, 0, 0), axis, 0.01, 2.0, rgba)
    return m


def step_terrain(seq, nseq, floor_z, box_half_heights, floor_rgba=(0.5, 0.5, 0.5, 1.0)) -> Markers:
    """The stepping terrain as 21 dynamic geoms per frame (tasks/stepping_task.py:320-334) from seq [F][20][>=4], nseq [F], floor_z [F] and
    the model's box half heights [20]: box i at seq[i][:3] - (0, 0, box_h), yaw seq[i][3], half extents (0.15, 1, box_h), colour (0.8, 0.8,
    0.8, 1); the boxes past the sequence at the reference's parking pose (0, 0, -1 - box_h); the floor plane at z = floor_z.  The model's
    own box and floor geoms are to be hidden (Renderer's hidden_geoms) when the terrain is drawn this way."""
    seq, nseq, floor_z = np.asarray(seq, dtype=np.float64), np.asarray(nseq).reshape(-1).astype(int), np.asarray(floor_z, dtype=np.float64).reshape(-1)
    bh = np.asarray(box_half_heights, dtype=np.float64).reshape(NBOX)
    m = Markers()
    for f in range(len(nseq)):
        for i in range(NBOX):
            step = seq[f, i, :4] if i < nseq[f] else np.array([0.0, 0.0, -1.0, 0.0])
            m.add(f, BOX, (0.15, 1.0, bh[i]), (0.8, 0.8, 0.8, 1.0), step[:3] - [0.0, 0.0, bh[i]], yaw_mat(step[3]))
        m.add(f, PLANE, (0, 0, 0), floor_rgba, (0.0, 0.0, floor_z[f]))
    return m
