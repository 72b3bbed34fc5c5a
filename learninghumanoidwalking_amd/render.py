"""Headless frames of a recorded motion: the host side of lhw_render_frames and lhw_render_scene (include/lhw.h), the HIP ray caster
for the analytic primitives the model loader accepts; markers.py builds the per-frame geoms (task markers, stepping terrain) of the second.

The reference's eval renders a 640 x 480 tracking camera once per control step through MuJoCo's GL renderer and writes a video
(rl/utils/eval.py:38-86).  Here the geoms of every frame are posed on the host in float64 (kinematics.geom_poses), expressed relative
to the frame's camera position before the cast to float32 -- a robot 50 m from the origin renders like one at the origin -- and the
device casts the rays.  Frames leave as PNG files written with zlib alone.  No pixel parity with MuJoCo's renderer is claimed: the
camera and the shading are the ones defined in include/lhw.h and in TrackingCamera below.
"""
from __future__ import annotations

import ctypes
import math
import struct
import zlib

import numpy as np
import torch

from . import _lib
from .kinematics import body_poses, geom_poses
from .model import Model, default_geom_rgba

CHUNK_BYTES = 64 << 20      # render() works in frame chunks whose image buffer stays below this

DEFAULT_SETTINGS = dict(fovy_deg=45.0, light_dir=(0.3, -0.5, 1.0), ambient=0.35, diffuse=0.65, background=(0.55, 0.70, 0.90),
                        checker_size=0.5, shadows=True, cull=True)


class TrackingCamera:
    """A camera that follows a body, with the reference's numbers (rl/utils/eval.py:50-52, 64: distance 4, elevation -20, lookat = body 1;
    azimuth 90 is MuJoCo's default, which the reference leaves).  Our own definition, in degrees and world axes (z up):

        forward  = (cos el cos az, cos el sin az, sin el)
        position = lookat - distance * forward              lookat = the origin of body `lookat_body` in that frame
        right    = normalize(forward x z),  up = right x forward

    `lookat`: a fixed world point instead of a body (then `lookat_body` is ignored)."""

    def __init__(self, distance=4.0, azimuth=90.0, elevation=-20.0, lookat_body=1, lookat=None):
        self.distance, self.azimuth, self.elevation, self.lookat_body = float(distance), float(azimuth), float(elevation), int(lookat_body)
        self.lookat = None if lookat is None else np.asarray(lookat, dtype=np.float64).reshape(3)

    def axes(self):
        """(right, up, forward), float64 unit vectors"""
        az, el = math.radians(self.azimuth), math.radians(self.elevation)
        fwd = np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])
        right = np.cross(fwd, [0.0, 0.0, 1.0])
        right /= np.linalg.norm(right)
        return right, np.cross(right, fwd), fwd

    def poses(self, body_xpos):
        """(position [F][3], rows [F][9] = right, up, forward) for body positions [F][nbody][3]"""
        right, up, fwd = self.axes()
        F = body_xpos.shape[0]
        look = body_xpos[:, self.lookat_body] if self.lookat is None else np.broadcast_to(self.lookat, (F, 3))
        return look - self.distance * fwd, np.broadcast_to(np.concatenate([right, up, fwd]), (F, 9)).copy()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Renderer:
    """Frames of `model` on `device`: uploads the static geom tables (type, size, colour) once; `render` poses and draws.

    `library`: a ctypes handle of another build of the C ABI that _lib.declare was applied to (None: the GPU library); only with one may
    `device` be a CPU device.  `settings`: the fields of LhwRenderSettings behind width / height (DEFAULT_SETTINGS); light_dir is
    normalised here.  `hidden_geoms`: geom ids drawn with alpha 0 (not drawn, no shadow)."""

    def __init__(self, model: Model | None, width=640, height=480, device: int | torch.device = 0, library=None, hidden_geoms=(), **settings):
        if model is not None:
            a = model.arrays
            gb = np.asarray(a["geom_bodyid"])
            rgba = model.geom_rgba if model.geom_rgba is not None else np.array([default_geom_rgba(t, b) for t, b in zip(a["geom_type"], gb)])
            rgba = np.array(rgba, dtype=np.float64).reshape(-1, 4)
            rgba[list(hidden_geoms), 3] = 0.0
            self._init_tables(a["geom_type"], a["geom_size"], rgba, width, height, device, library, settings)
        self.model = model

    @classmethod
    def from_geoms(cls, geom_type, geom_size, geom_rgba, width=640, height=480, device: int | torch.device = 0, library=None, **settings):
        """A renderer of loose geoms (no model, no kinematics): `render_geoms` takes their poses."""
        r = cls(None)
        r._init_tables(geom_type, geom_size, geom_rgba, width, height, device, library, settings)
        return r

    def _init_tables(self, geom_type, geom_size, geom_rgba, width, height, device, library, settings):
        if library is None and not torch.cuda.is_available():
            raise _lib.LhwError(-5, "no GPU visible: the renderer has no CPU fallback")
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if library is None and self.device.type != "cuda":
            raise _lib.LhwError(-5, f"device {self.device}: the renderer has no CPU fallback")
        self._L = _lib.lib() if library is None else library
        if getattr(self._L, "lhw_render_frames", None) is None:
            raise _lib.LhwError(-4, "this build of the library does not export lhw_render_frames")
        unknown = set(settings) - set(DEFAULT_SETTINGS)
        if unknown:
            raise TypeError(f"unknown render settings {sorted(unknown)}: the settings are {sorted(DEFAULT_SETTINGS)}")
        cfg = dict(DEFAULT_SETTINGS, **settings)
        self.width, self.height = int(width), int(height)
        s = self.settings = _lib.LhwRenderSettings()
        s.width, s.height, s.fovy_deg = self.width, self.height, float(cfg["fovy_deg"])
        light = np.asarray(cfg["light_dir"], dtype=np.float64)
        for k in range(3):
            s.light_dir[k] = float(light[k] / np.linalg.norm(light))
            s.background[k] = float(cfg["background"][k])
        s.ambient, s.diffuse, s.checker_size = float(cfg["ambient"]), float(cfg["diffuse"]), float(cfg["checker_size"])
        s.shadows, s.cull = int(bool(cfg["shadows"])), int(bool(cfg["cull"]))
        self.n_geoms = int(np.asarray(geom_type).size)
        up = lambda x, dt, shape: torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=dt).reshape(shape))).to(self.device)
        self._type = up(geom_type, np.int32, (self.n_geoms,))
        self._size = up(geom_size, np.float32, (self.n_geoms, 3))
        self._rgba = up(geom_rgba, np.float32, (self.n_geoms, 4))

    @property
    def frames_per_chunk(self) -> int:
        return max(1, (CHUNK_BYTES - 1) // (self.width * self.height * 3))

    def upload(self, pos, mat, cam_pos, cam_rows):
        """The per-frame device buffers of lhw_render_frames -- (geom_pos [F][G][3] relative to the camera, geom_mat [F][G][9], cam [F][12]),
        float32 -- from float64 world poses; the subtraction and the checkerboard's camera offset are done here, in float64."""
        pos = np.asarray(pos, dtype=np.float64)
        F, G = pos.shape[0], self.n_geoms
        cam_pos = np.asarray(cam_pos, dtype=np.float64).reshape(F, 3)
        rel = pos.reshape(F, G, 3) - cam_pos[:, None, :]
        cam = np.zeros((F, 12), dtype=np.float64)
        cam[:, :9] = np.asarray(cam_rows, dtype=np.float64).reshape(F, 9)
        c = float(self.settings.checker_size)
        if c > 0.0:
            cam[:, 9:11] = np.mod(cam_pos[:, :2], 2.0 * c)
        return tuple(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(self.device)
                     for x in (rel, np.asarray(mat, dtype=np.float64).reshape(F, G, 9), cam))

    def draw(self, frames, rgb, hit=None, depth=None):
        """One lhw_render_frames call on the current stream: `frames` from upload(), outputs [F][H][W][3] uint8 / [F][H][W] int32 / float32"""
        d_pos, d_mat, d_cam = frames
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream) if self.device.type == "cuda" else None
        _lib.check(self._L.lhw_render_frames(ctypes.byref(self.settings), self.n_geoms, _ptr(self._type), _ptr(self._size), _ptr(self._rgba),
                                             d_pos.shape[0], _ptr(d_pos), _ptr(d_mat), _ptr(d_cam), _ptr(rgb), _ptr(hit), _ptr(depth), stream), self._L)

    def render_geoms(self, pos, mat, cam_pos, cam_rows, aux=False, out=None):
        """Draw F frames of posed geoms: pos [F][G][3] / mat [F][G][9] world poses and cam_pos [F][3] / cam_rows [F][9] (right, up,
        forward) in float64 numpy.  Returns the uint8 tensor [F][H][W][3] on the renderer's device; aux=True: (rgb, hit int32 [F][H][W],
        depth float32 [F][H][W]) as include/lhw.h defines them.  `out`: (rgb, hit or None, depth or None) tensors to draw into (one launch,
        no chunking)."""
        pos, mat, cam_pos, cam_rows = (np.asarray(x, dtype=np.float64) for x in (pos, mat, cam_pos, cam_rows))
        F, H, W = pos.shape[0], self.height, self.width
        if out is not None:
            rgb, hit, depth = out
            chunk = max(F, 1)
        else:
            rgb = _lib.empty(F, H, W, 3, dtype=torch.uint8, device=self.device)
            hit = _lib.empty(F, H, W, dtype=torch.int32, device=self.device) if aux else None
            depth = _lib.empty(F, H, W, dtype=torch.float32, device=self.device) if aux else None
            chunk = self.frames_per_chunk
        for f0 in range(0, F, chunk):
            f1 = min(F, f0 + chunk)
            self.draw(self.upload(pos[f0:f1], mat[f0:f1], cam_pos.reshape(F, 3)[f0:f1], cam_rows.reshape(F, 9)[f0:f1]), rgb[f0:f1],
                      None if hit is None else hit[f0:f1], None if depth is None else depth[f0:f1])
        return (rgb, hit, depth) if aux or out is not None else rgb

    def upload_dynamic(self, dynamic, cam_pos):
        """The per-frame device tables of lhw_render_scene's dynamic geoms -- (type [F][M] int32, size [F][M][3], rgba [F][M][4], pos
        [F][M][3] relative to the camera, mat [F][M][9]), float32 -- from `dynamic`: a markers.Markers, or a dict of numpy arrays type
        [F][M], size, rgba, pos (world, float64), mat.  The subtraction is done here, in float64."""
        cam_pos = np.asarray(cam_pos, dtype=np.float64).reshape(-1, 3)
        F = cam_pos.shape[0]
        d = dynamic.arrays(F) if hasattr(dynamic, "arrays") else dynamic
        t = np.asarray(d.get("type", np.zeros((F, 0))), dtype=np.int32).reshape(F, -1)
        M = t.shape[1]
        f64 = lambda k, n: np.asarray(d[k], dtype=np.float64).reshape(F, M, n) if M else np.zeros((F, 0, n))
        rel = f64("pos", 3) - cam_pos[:, None, :]
        up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(self.device)
        return up(t, np.int32), up(f64("size", 3), np.float32), up(f64("rgba", 4), np.float32), up(rel, np.float32), up(f64("mat", 9), np.float32)

    def draw_scene(self, frames, dyn, rgb, hit=None, depth=None, layers=None, layer_hit=None):
        """One lhw_render_scene call on the current stream: `frames` from upload(), `dyn` from upload_dynamic(), outputs as draw()'s plus
        layers / layer_hit [F][H][W] int32"""
        if getattr(self._L, "lhw_render_scene", None) is None:
            raise _lib.LhwError(-4, "this build of the library does not export lhw_render_scene")
        d_pos, d_mat, d_cam = frames
        d_type, d_size, d_rgba, d_dpos, d_dmat = dyn
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream) if self.device.type == "cuda" else None
        _lib.check(self._L.lhw_render_scene(ctypes.byref(self.settings), self.n_geoms, _ptr(self._type), _ptr(self._size), _ptr(self._rgba),
                                            d_type.shape[1], _ptr(d_type), _ptr(d_size), _ptr(d_rgba), d_cam.shape[0], _ptr(d_pos), _ptr(d_mat),
                                            _ptr(d_dpos), _ptr(d_dmat), _ptr(d_cam), _ptr(rgb), _ptr(hit), _ptr(depth), _ptr(layers), _ptr(layer_hit),
                                            stream), self._L)

    def render_scene(self, pos, mat, cam_pos, cam_rows, dynamic=None, aux=False, out=None):
        """render_geoms plus per-frame geoms.  `dynamic` None: exactly render_geoms (lhw_render_frames, the bytes its callers get today).
        Otherwise -- a markers.Markers or the dict upload_dynamic takes, an empty one included -- the frames go through lhw_render_scene:
        the dynamic geoms get the ids G + m, alpha in (0, 1) is translucent, and aux=True returns (rgb, hit, depth, layers, layer_hit).
        `out`: the five tensors (the last four may be None) to draw into, one launch."""
        if dynamic is None:
            return self.render_geoms(pos, mat, cam_pos, cam_rows, aux=aux, out=out)
        pos, mat, cam_pos, cam_rows = (np.asarray(x, dtype=np.float64) for x in (pos, mat, cam_pos, cam_rows))
        F, H, W = cam_pos.reshape(-1, 3).shape[0], self.height, self.width
        pos, mat = pos.reshape(F, self.n_geoms, 3), mat.reshape(F, self.n_geoms, 9)
        if out is not None:
            bufs, chunk = list(out), max(F, 1)
        else:
            i32 = lambda: _lib.empty(F, H, W, dtype=torch.int32, device=self.device) if aux else None
            bufs = [_lib.empty(F, H, W, 3, dtype=torch.uint8, device=self.device), i32(),
                    _lib.empty(F, H, W, dtype=torch.float32, device=self.device) if aux else None, i32(), i32()]
            chunk = self.frames_per_chunk
        d = dynamic.arrays(F) if hasattr(dynamic, "arrays") else dynamic
        for f0 in range(0, F, chunk):
            f1 = min(F, f0 + chunk)
            cp = cam_pos.reshape(F, 3)[f0:f1]
            self.draw_scene(self.upload(pos[f0:f1], mat[f0:f1], cp, cam_rows.reshape(F, 9)[f0:f1]),
                            self.upload_dynamic({k: np.asarray(v)[f0:f1] for k, v in d.items()}, cp), *(None if b is None else b[f0:f1] for b in bufs))
        return tuple(bufs) if aux or out is not None else bufs[0]

    def render(self, qpos, camera: TrackingCamera | None = None, aux=False, markers=None):
        """Frames of the poses qpos [F][nq] (or [nq]) seen by `camera` (default: TrackingCamera()): uint8 tensor [F][H][W][3].  `markers`: a
        markers.Markers (or upload_dynamic's dict) of per-frame geoms drawn with the model's, through lhw_render_scene (render_scene)."""
        if self.model is None:
            raise ValueError("a renderer of loose geoms has no kinematics: use render_geoms")
        camera = TrackingCamera() if camera is None else camera
        q = np.atleast_2d(np.asarray(qpos, dtype=np.float64))
        pos, mat = geom_poses(self.model, q)
        cam_pos, cam_rows = camera.poses(body_poses(self.model, q)[0])
        return self.render_scene(pos, mat, cam_pos, cam_rows, dynamic=markers, aux=aux)


def write_png(path, array) -> None:
    """An 8-bit PNG of a uint8 array [H][W][3] (RGB) or [H][W] (grey), written with zlib and struct alone (filter 0 on every row)."""
    a = np.ascontiguousarray(array.cpu().numpy() if isinstance(array, torch.Tensor) else array)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"write_png takes a uint8 array [H][W][3] or [H][W], got {a.dtype} {a.shape}")
    h, w = a.shape[:2]
    rows = np.concatenate([np.zeros((h, 1), dtype=np.uint8), a.reshape(h, -1)], axis=1)

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2 if a.ndim == 3 else 0, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b""))
