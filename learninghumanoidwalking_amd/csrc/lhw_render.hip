// Headless eval frames (include/lhw.h: lhw_render_frames): a ray caster for the analytic primitives the model loader accepts -- the
// rendering half of the reference's eval (rl/utils/eval.py:38-67: a tracking camera, one frame per control step) without GL and
// without CPU MuJoCo.
//
// Lane mapping: one wavefront per 8 x 8 pixel tile of one frame (grid = tiles x frames, block 64).  There are at most 64 geoms and 64
// lanes, so the tile's work list costs one pass: lane g takes geom g, moves the camera (the origin: geom positions arrive relative to
// it) and the light direction into the geom's frame, leaves the record in LDS, tests the geom's bounding sphere against the four side
// planes of the tile's frustum, and a ballot gives the tile's candidate mask.  The wave then walks the set bits of that mask -- a
// wave-uniform loop, the record read from LDS at one address (a broadcast) -- and every lane intersects its own pixel's ray in the
// geom's local frame, where every primitive is axis-aligned.  Shadow rays leave the tile's frustum: they walk the mask of all drawn
// geoms, and a lane stops testing at its first hit.  The tile's 192 colour bytes are collected in LDS so that full tiles leave as six
// dwords per row.  Arithmetic is float32; the quadratics are solved from the ray's closest approach to the centre / axis (compare
// |o - (o.d) d|^2 with r^2), which does not cancel for a small geom far away the way b^2 - 4ac does.
#include <math.h>

#include <vector>

#include "lhw_internal.h"

namespace {

enum { G_PLANE = 0, G_SPHERE = 2, G_CAPSULE = 3, G_ELLIPSOID = 4, G_CYLINDER = 5, G_BOX = 6 };   // mjtGeom, as geom_type of the packed model
enum { REC = 24 };   // floats per geom record in LDS: camera in the geom frame (3), rotation (9), size (3), light direction in the geom frame (3), type, pad

struct RenderArgs {
  int W, H, G, tiles_x, tiles;
  float tan_half, aspect;
  float light[3], ambient, diffuse, bg[3], checker;
  int shadows, cull;
  const int32_t* type;
  const float *size, *rgba, *pos, *mat, *cam;
  uint8_t* rgb;
  int32_t* hit;
  float* depth;
};

struct V3 { float x, y, z; };
__device__ __forceinline__ float dot3(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
// R^T v and R v for a row-major rotation (columns = the geom's axes in the world)
__device__ __forceinline__ V3 to_local(const float* R, V3 v) {
  return V3{R[0] * v.x + R[3] * v.y + R[6] * v.z, R[1] * v.x + R[4] * v.y + R[7] * v.z, R[2] * v.x + R[5] * v.y + R[8] * v.z};
}
__device__ __forceinline__ V3 to_world(const float* R, V3 v) {
  return V3{R[0] * v.x + R[1] * v.y + R[2] * v.z, R[3] * v.x + R[4] * v.y + R[5] * v.z, R[6] * v.x + R[7] * v.y + R[8] * v.z};
}

__device__ __forceinline__ void take(float t, int part, float& best, int& best_part) {
  if (t > 0.f && t < best) { best = t; best_part = part; }
}

// circle / sphere of radius r around the origin in `dim` dimensions (2: the z components are passed as 0), direction of squared length a:
// the two ray parameters from the closest approach (no cancellation: q2 is computed from the closest point itself)
__device__ __forceinline__ bool roots(V3 o, V3 d, float a, float r, float& t0, float& t1) {
  if (!(a > 1e-20f)) return false;
  const float tc = -dot3(o, d) / a;
  const V3 q{o.x + tc * d.x, o.y + tc * d.y, o.z + tc * d.z};
  const float h2 = r * r - dot3(q, q);
  if (h2 < 0.f) return false;
  const float h = sqrtf(h2 / a);
  t0 = tc - h; t1 = tc + h;
  return true;
}

// nearest surface point with t > 0 of the ray o + t d (|d| = 1, geom frame) on a geom of `type` / size s; `part` as include/lhw.h
__device__ bool intersect(int type, V3 s, V3 o, V3 d, float& t_out, int& part_out) {
  float best = INFINITY;
  int part = 0;
  float t0, t1;
  if (type == G_PLANE) {
    if (d.z != 0.f) take(-o.z / d.z, 0, best, part);
  } else if (type == G_SPHERE) {
    if (roots(o, d, 1.f, s.x, t0, t1)) { take(t0, 0, best, part); take(t1, 0, best, part); }
  } else if (type == G_ELLIPSOID) {
    const V3 os{o.x / s.x, o.y / s.y, o.z / s.z}, ds{d.x / s.x, d.y / s.y, d.z / s.z};
    if (roots(os, ds, dot3(ds, ds), 1.f, t0, t1)) { take(t0, 0, best, part); take(t1, 0, best, part); }
  } else if (type == G_CAPSULE || type == G_CYLINDER) {
    const float r = s.x, hl = s.y;
    const V3 o2{o.x, o.y, 0.f}, d2{d.x, d.y, 0.f};
    if (roots(o2, d2, d.x * d.x + d.y * d.y, r, t0, t1)) {      // the body: |z| <= hl
      if (fabsf(o.z + t0 * d.z) <= hl) take(t0, 0, best, part);
      if (fabsf(o.z + t1 * d.z) <= hl) take(t1, 0, best, part);
    }
    for (int e = 0; e < 2; e++) {
      const float ze = e ? hl : -hl;
      if (type == G_CAPSULE) {                                  // a cap: the half of the sphere around the end point that lies beyond it
        const V3 oc{o.x, o.y, o.z - ze};
        if (roots(oc, d, 1.f, r, t0, t1)) {
          const float z0 = oc.z + t0 * d.z, z1 = oc.z + t1 * d.z;
          if (e ? z0 > 0.f : z0 < 0.f) take(t0, 1 + e, best, part);
          if (e ? z1 > 0.f : z1 < 0.f) take(t1, 1 + e, best, part);
        }
      } else if (d.z != 0.f) {                                  // a disc
        const float t = (ze - o.z) / d.z;
        const float x = o.x + t * d.x, y = o.y + t * d.y;
        if (x * x + y * y <= r * r) take(t, 1 + e, best, part);
      }
    }
  } else {      // G_BOX: slabs
    const float oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z}, ss[3] = {s.x, s.y, s.z};
    float tn = -INFINITY, tf = INFINITY;
    int fn = 0, ff = 0;
    bool miss = false;
    for (int a = 0; a < 3; a++) {
      if (dd[a] == 0.f) { miss = miss || fabsf(oo[a]) > ss[a]; continue; }
      const float inv = 1.f / dd[a];
      const float ta = (-ss[a] - oo[a]) * inv, tb = (ss[a] - oo[a]) * inv;      // the -a face, the +a face
      const bool pos = dd[a] > 0.f;                                            // entering through -a
      const float lo = pos ? ta : tb, hi = pos ? tb : ta;
      if (lo > tn) { tn = lo; fn = 2 * a + (pos ? 0 : 1); }
      if (hi < tf) { tf = hi; ff = 2 * a + (pos ? 1 : 0); }
    }
    if (!miss && tn <= tf) { take(tn, fn, best, part); take(tf, ff, best, part); }
  }
  t_out = best; part_out = part;
  return best < INFINITY;
}

// outward unit normal in the geom frame at the surface point p of `part`; o: the ray origin (a plane shows the side the viewer is on)
__device__ V3 normal_local(int type, V3 s, V3 p, int part, V3 o) {
  V3 n{0.f, 0.f, 1.f};
  if (type == G_PLANE) n.z = o.z >= 0.f ? 1.f : -1.f;
  else if (type == G_SPHERE) n = p;
  else if (type == G_ELLIPSOID) n = V3{p.x / (s.x * s.x), p.y / (s.y * s.y), p.z / (s.z * s.z)};
  else if (type == G_BOX) { const float sg = (part & 1) ? 1.f : -1.f; n = V3{part < 2 ? sg : 0.f, (part >> 1) == 1 ? sg : 0.f, part >= 4 ? sg : 0.f}; }
  else if (part == 0) n = V3{p.x, p.y, 0.f};
  else if (type == G_CAPSULE) n = V3{p.x, p.y, p.z - (part == 2 ? s.y : -s.y)};
  else n.z = part == 2 ? 1.f : -1.f;
  const float l = sqrtf(dot3(n, n));
  return l > 0.f ? V3{n.x / l, n.y / l, n.z / l} : V3{0.f, 0.f, 1.f};
}

__device__ __forceinline__ float bound_radius(int type, V3 s) {
  if (type == G_SPHERE) return s.x;
  if (type == G_CAPSULE) return s.x + s.y;
  if (type == G_CYLINDER) return sqrtf(s.x * s.x + s.y * s.y);
  if (type == G_ELLIPSOID) return fmaxf(s.x, fmaxf(s.y, s.z));
  return sqrtf(dot3(s, s));
}

__device__ __forceinline__ uint8_t to_byte(float c) { return (uint8_t)(int)floorf(255.f * fminf(1.f, fmaxf(0.f, c)) + 0.5f); }

__global__ void __launch_bounds__(64) render_kernel(RenderArgs a) {
  __shared__ float rec[LHW_RENDER_MAX_GEOMS * REC];
  __shared__ uint32_t tile_rgb[48];      // [8 rows][24 bytes]
  LHW_LDS_POISON(rec);
  LHW_LDS_POISON(tile_rgb);
  const int lane = threadIdx.x;
  const int f = blockIdx.x / a.tiles, tile = blockIdx.x - f * a.tiles;
  const int x0 = (tile % a.tiles_x) * 8, y0 = (tile / a.tiles_x) * 8;
  const float* cam = a.cam + (size_t)f * 12;
  const V3 right{cam[0], cam[1], cam[2]}, up{cam[3], cam[4], cam[5]}, fwd{cam[6], cam[7], cam[8]};
  const V3 light{a.light[0], a.light[1], a.light[2]};

  // ---- lane g: geom g's record, and whether its bounding sphere reaches the tile's frustum
  bool drawn = false, cand = false;
  if (lane < a.G) {
    const int g = lane;
    const float* P = a.pos + ((size_t)f * a.G + g) * 3;
    const float* R = a.mat + ((size_t)f * a.G + g) * 9;
    float* r = rec + g * REC;
    const int type = a.type[g];
    const V3 p{P[0], P[1], P[2]}, s{a.size[3 * g], a.size[3 * g + 1], a.size[3 * g + 2]};
    float Rl[9];
    for (int k = 0; k < 9; k++) Rl[k] = R[k];
    const V3 o = to_local(Rl, V3{-p.x, -p.y, -p.z}), ll = to_local(Rl, light);
    r[0] = o.x; r[1] = o.y; r[2] = o.z;
    for (int k = 0; k < 9; k++) r[3 + k] = Rl[k];
    r[12] = s.x; r[13] = s.y; r[14] = s.z;
    r[15] = ll.x; r[16] = ll.y; r[17] = ll.z;
    r[18] = (float)type;
    drawn = a.rgba[4 * g + 3] != 0.f;
    cand = drawn;
    if (drawn && a.cull && type != G_PLANE) {
      const float cx = dot3(right, p), cy = dot3(up, p), cz = dot3(fwd, p);
      const float m = 1.01f * bound_radius(type, s) + 1e-4f * (1.f + fabsf(cx) + fabsf(cy) + fabsf(cz));
      const float kx = a.tan_half * a.aspect, ky = a.tan_half;
      const float xl = kx * (2.f * (float)x0 / (float)a.W - 1.f), xr = kx * (2.f * (float)(x0 + 8) / (float)a.W - 1.f);
      const float yt = -ky * (2.f * (float)y0 / (float)a.H - 1.f), yb = -ky * (2.f * (float)(y0 + 8) / (float)a.H - 1.f);
      cand = (cx - xl * cz >= -m * sqrtf(1.f + xl * xl)) && (xr * cz - cx >= -m * sqrtf(1.f + xr * xr)) &&
             (cy - yb * cz >= -m * sqrtf(1.f + yb * yb)) && (yt * cz - cy >= -m * sqrtf(1.f + yt * yt));
    }
  }
  const unsigned long long drawn_mask = __ballot(drawn);
  unsigned long long mask = __ballot(cand);
  __syncthreads();

  // ---- primary rays: lane = pixel (lane % 8, lane / 8) of the tile
  const int px = x0 + (lane & 7), py = y0 + (lane >> 3);
  const float sx = a.tan_half * a.aspect * (2.f * ((float)px + 0.5f) / (float)a.W - 1.f);
  const float sy = -a.tan_half * (2.f * ((float)py + 0.5f) / (float)a.H - 1.f);
  V3 d{fwd.x + sx * right.x + sy * up.x, fwd.y + sx * right.y + sy * up.y, fwd.z + sx * right.z + sy * up.z};
  {
    const float inv = 1.f / sqrtf(dot3(d, d));
    d = V3{d.x * inv, d.y * inv, d.z * inv};
  }
  float best = INFINITY;
  int best_g = -1, best_part = 0;
  while (mask) {
    const int g = __ffsll(mask) - 1;
    mask &= mask - 1;
    const float* r = rec + g * REC;
    float t;
    int part;
    if (intersect((int)r[18], V3{r[12], r[13], r[14]}, V3{r[0], r[1], r[2]}, to_local(r + 3, d), t, part) && t < best) {
      best = t; best_g = g; best_part = part;
    }
  }

  // ---- shading
  V3 col{a.bg[0], a.bg[1], a.bg[2]};
  V3 so{0.f, 0.f, 0.f};      // shadow ray origin (world, relative to the camera)
  bool want_shadow = false;
  float ndl = 0.f;
  if (best_g >= 0) {
    const float* r = rec + best_g * REC;
    const int type = (int)r[18];
    const V3 s{r[12], r[13], r[14]}, o{r[0], r[1], r[2]}, dl = to_local(r + 3, d);
    const V3 pl{o.x + best * dl.x, o.y + best * dl.y, o.z + best * dl.z};
    const V3 n = to_world(r + 3, normal_local(type, s, pl, best_part, o));
    ndl = fmaxf(0.f, dot3(n, light));
    const V3 hw{best * d.x, best * d.y, best * d.z};
    const float* c = a.rgba + 4 * best_g;
    col = V3{c[0], c[1], c[2]};
    if (type == G_PLANE && a.checker > 0.f) {
      const int ix = (int)floorf((cam[9] + hw.x) / a.checker), iy = (int)floorf((cam[10] + hw.y) / a.checker);
      if ((ix + iy) & 1) col = V3{0.8f * col.x, 0.8f * col.y, 0.8f * col.z};
    }
    so = V3{hw.x + 1e-3f * n.x, hw.y + 1e-3f * n.y, hw.z + 1e-3f * n.z};
    want_shadow = a.shadows != 0 && ndl > 0.f;
  }
  if (a.shadows) {
    bool open = want_shadow;      // still looking for an occluder
    unsigned long long sm = drawn_mask;
    while (sm && __any(open)) {
      const int g = __ffsll(sm) - 1;
      sm &= sm - 1;
      if (open) {
        const float* r = rec + g * REC;
        const V3 o{r[0], r[1], r[2]};      // o = -R^T p, so R^T (so - p) = R^T so + o
        const V3 sl = to_local(r + 3, so);
        float t;
        int part;
        if (intersect((int)r[18], V3{r[12], r[13], r[14]}, V3{o.x + sl.x, o.y + sl.y, o.z + sl.z}, V3{r[15], r[16], r[17]}, t, part)) open = false;
      }
    }
    if (want_shadow && !open) ndl = 0.f;
  }
  if (best_g >= 0) {
    const float sh = a.ambient + a.diffuse * ndl;
    col = V3{col.x * sh, col.y * sh, col.z * sh};
  }

  // ---- output: hit / depth per lane, colours through LDS
  const bool inside = px < a.W && py < a.H;
  const size_t pix = ((size_t)f * a.H + py) * a.W + px;
  if (inside) {
    if (a.hit) a.hit[pix] = best_g >= 0 ? best_g * 8 + best_part : -1;
    if (a.depth) a.depth[pix] = best;
  }
  uint8_t* tb = reinterpret_cast<uint8_t*>(tile_rgb);
  tb[3 * lane] = to_byte(col.x); tb[3 * lane + 1] = to_byte(col.y); tb[3 * lane + 2] = to_byte(col.z);
  __syncthreads();
  const int rows = min(8, a.H - y0), cols = min(8, a.W - x0);
  uint8_t* out = a.rgb + (((size_t)f * a.H + y0) * a.W + x0) * 3;
  const size_t pitch = (size_t)a.W * 3;
  if (cols == 8 && ((uintptr_t)out & 3) == 0 && (pitch & 3) == 0) {      // a full-width tile of dword-aligned rows: six dwords per row
    if (lane < 6 * rows) {
      const int row = lane / 6, k = lane - 6 * row;
      reinterpret_cast<uint32_t*>(out + row * pitch)[k] = tile_rgb[6 * row + k];
    }
  } else {
    for (int b = lane; b < 192; b += 64) {
      const int row = b / 24, k = b - 24 * row;
      if (row < rows && k < 3 * cols) out[row * pitch + k] = tb[b];
    }
  }
}

}  // namespace

extern "C" int lhw_render_frames(const LhwRenderSettings* s, int32_t G, const int32_t* geom_type_dev, const float* geom_size_dev,
                                 const float* geom_rgba_dev, int32_t F, const float* geom_pos_dev, const float* geom_mat_dev,
                                 const float* cam_dev, uint8_t* rgb_dev, int32_t* hit_dev, float* depth_dev, void* stream) {
  if (!s) return lhw_fail(LHW_ERR_ARG, "lhw_render_frames: settings is NULL");
  if (G > LHW_RENDER_MAX_GEOMS) return lhw_fail(LHW_ERR_UNSUPPORTED, "lhw_render_frames: %d geoms, one wavefront holds %d", G, LHW_RENDER_MAX_GEOMS);
  if (G < 0 || F < 0) return lhw_fail(LHW_ERR_ARG, "lhw_render_frames: G = %d, F = %d", G, F);
  if (s->width < 1 || s->height < 1) return lhw_fail(LHW_ERR_ARG, "lhw_render_frames: image size %d x %d", s->width, s->height);
  if (!(s->fovy_deg > 0.f && s->fovy_deg < 180.f)) return lhw_fail(LHW_ERR_ARG, "lhw_render_frames: fovy_deg = %g must lie in (0, 180)", (double)s->fovy_deg);
  if (!(s->checker_size >= 0.f)) return lhw_fail(LHW_ERR_ARG, "lhw_render_frames: checker_size = %g", (double)s->checker_size);
  if (!rgb_dev || !cam_dev || (G && (!geom_type_dev || !geom_size_dev || !geom_rgba_dev || !geom_pos_dev || !geom_mat_dev)))
    return lhw_fail(LHW_ERR_ARG, "lhw_render_frames: a required buffer is NULL");
  hipStream_t st = (hipStream_t)stream;
  if (G) {      // the static tables once on the host: a wrong type or size is refused before anything is written
    std::vector<int32_t> type(G);
    std::vector<float> size(3 * (size_t)G), rgba(4 * (size_t)G);
    HIPCHK(hipMemcpyAsync(type.data(), geom_type_dev, sizeof(int32_t) * G, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(size.data(), geom_size_dev, sizeof(float) * 3 * G, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(rgba.data(), geom_rgba_dev, sizeof(float) * 4 * G, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int g = 0; g < G; g++) {
      const int t = type[g];
      if (t != G_PLANE && t != G_SPHERE && t != G_CAPSULE && t != G_ELLIPSOID && t != G_CYLINDER && t != G_BOX)
        return lhw_fail(LHW_ERR_ARG, "lhw_render_frames: geom %d has type %d (plane 0, sphere 2, capsule 3, ellipsoid 4, cylinder 5, box 6)", g, t);
      const int need = t == G_PLANE ? 0 : (t == G_SPHERE ? 1 : ((t == G_CAPSULE || t == G_CYLINDER) ? 2 : 3));
      for (int k = 0; k < need; k++)
        if (rgba[4 * g + 3] != 0.f && !(size[3 * g + k] > 0.f))
          return lhw_fail(LHW_ERR_ARG, "lhw_render_frames: geom %d (type %d) has size[%d] = %g", g, t, k, (double)size[3 * g + k]);
    }
  }
  if (F == 0) return LHW_OK;
  RenderArgs a;
  a.W = s->width; a.H = s->height; a.G = G;
  a.tiles_x = (a.W + 7) / 8;
  a.tiles = a.tiles_x * ((a.H + 7) / 8);
  if ((long long)a.tiles * F > 0x7fffffffLL) return lhw_fail(LHW_ERR_ARG, "lhw_render_frames: %d frames of %d tiles exceed one launch", F, a.tiles);
  a.tan_half = (float)tan(0.5 * (double)s->fovy_deg * 3.14159265358979323846 / 180.0);
  a.aspect = (float)((double)a.W / (double)a.H);
  for (int k = 0; k < 3; k++) { a.light[k] = s->light_dir[k]; a.bg[k] = s->background[k]; }
  a.ambient = s->ambient; a.diffuse = s->diffuse; a.checker = s->checker_size;
  a.shadows = s->shadows; a.cull = s->cull;
  a.type = geom_type_dev; a.size = geom_size_dev; a.rgba = geom_rgba_dev; a.pos = geom_pos_dev; a.mat = geom_mat_dev; a.cam = cam_dev;
  a.rgb = rgb_dev; a.hit = hit_dev; a.depth = depth_dev;
  hipLaunchKernelGGL(render_kernel, dim3((unsigned)(a.tiles * F)), dim3(64), 0, st, a);
  HIPCHK(hipGetLastError());
  return LHW_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// lhw_render_scene (include/lhw.h): the same ray caster with per-frame ("dynamic") geoms behind the static ones, up to 256 geoms,
// translucent layers and a cone -- the task markers and the stepping terrain of the reference's eval.
//
// Lane mapping: still one wavefront per 8 x 8 tile.  The geom set is walked in PASSES = ceil((G + M) / 64) passes: in pass p lane l
// builds the record of geom 64 p + l and tests its bounding sphere against the tile's frustum, one ballot per pass gives the pass's
// candidate mask and a second one its mask of opaque drawn geoms (the occluders of the shadow rays).  All records stay in LDS
// (PASSES x 6 KB: the kernel is instantiated per pass count, so a scene of 64 geoms keeps the 6 KB workgroup of render_kernel), so
// that the shadow loop and the layer shading reach the geoms of every pass.  The masks are wave-uniform and stay in scalar registers.
// A lane keeps its nearest eight translucent surface points in registers, sorted by an unrolled compare-and-swap insertion; those
// in front of the nearest opaque surface -- a prefix of the sorted list -- are shaded and composited front to back.
// The primitives, the shading expressions and the output path are render_kernel's own, so alpha-1 scenes of at most 64 geoms get its values.
namespace {

enum { G_CONE = LHW_RENDER_CONE, PASS = 64, MAX_PASSES = LHW_RENDER_SCENE_MAX_GEOMS / PASS, LAYERS = LHW_RENDER_MAX_LAYERS };

struct SceneArgs {
  RenderArgs r;      // the static geoms (r.G of them) and everything shared with render_kernel
  int M;
  const int32_t* dtype;
  const float *dsize, *drgba, *dpos, *dmat;
  int32_t *layers, *layer_hit;
};

// cone of base radius s.x at z = -s.y and apex at z = +s.y.  With z measured from the apex the lateral surface is q(v) = x^2 + y^2 - k^2 z^2 = 0,
// k = r / (2 hl): the ray parameters come from the point of the ray where q is stationary, tc = -B(o, d) / q(d), and from q at that point
// (for a thin cone far away it lies next to the axis: both terms of q are of the size of r^2, not of the distance squared)
__device__ bool intersect_cone(V3 s, V3 o, V3 d, float& t_out, int& part_out) {
  const float r = s.x, hl = s.y, k = r / (2.f * hl), k2 = k * k;
  float best = INFINITY;
  int part = 0;
  const V3 oa{o.x, o.y, o.z - hl};
  const float a = d.x * d.x + d.y * d.y - k2 * d.z * d.z;
  const float b = oa.x * d.x + oa.y * d.y - k2 * oa.z * d.z;
  if (fabsf(a) > 1e-7f) {
    const float tc = -b / a;
    const V3 q{oa.x + tc * d.x, oa.y + tc * d.y, oa.z + tc * d.z};
    const float h2 = -(q.x * q.x + q.y * q.y - k2 * q.z * q.z) / a;
    if (h2 >= 0.f) {
      const float h = sqrtf(h2);
      const float t0 = tc - h, t1 = tc + h;
      const float z0 = oa.z + t0 * d.z, z1 = oa.z + t1 * d.z;      // the nappe below the apex, down to the base
      if (z0 <= 0.f && z0 >= -2.f * hl) take(t0, 0, best, part);
      if (z1 <= 0.f && z1 >= -2.f * hl) take(t1, 0, best, part);
    }
  } else if (b != 0.f) {                                          // the ray runs along a generator's direction: one crossing
    const float t = -(oa.x * oa.x + oa.y * oa.y - k2 * oa.z * oa.z) / (2.f * b);
    const float z = oa.z + t * d.z;
    if (z <= 0.f && z >= -2.f * hl) take(t, 0, best, part);
  }
  if (d.z != 0.f) {                                               // the base disc
    const float t = (-hl - o.z) / d.z;
    const float x = o.x + t * d.x, y = o.y + t * d.y;
    if (x * x + y * y <= r * r) take(t, 1, best, part);
  }
  t_out = best; part_out = part;
  return best < INFINITY;
}

__device__ __forceinline__ bool intersect_scene(int type, V3 s, V3 o, V3 d, float& t, int& part) {
  return type == G_CONE ? intersect_cone(s, o, d, t, part) : intersect(type, s, o, d, t, part);
}

__device__ __forceinline__ V3 normal_scene(int type, V3 s, V3 p, int part, V3 o) {
  if (type != G_CONE) return normal_local(type, s, p, part, o);
  if (part == 1) return V3{0.f, 0.f, -1.f};
  const float rho = sqrtf(p.x * p.x + p.y * p.y);
  const V3 n{p.x, p.y, rho * s.x / (2.f * s.y)};
  const float l = sqrtf(dot3(n, n));
  return l > 0.f ? V3{n.x / l, n.y / l, n.z / l} : V3{0.f, 0.f, 1.f};
}

// m[p] for a wave-uniform p: the four pass masks are scalars, not an indexed array (which the compiler would keep in scratch)
__device__ __forceinline__ unsigned long long pick(int p, unsigned long long m0, unsigned long long m1, unsigned long long m2, unsigned long long m3) {
  return p == 0 ? m0 : (p == 1 ? m1 : (p == 2 ? m2 : m3));
}

// pass p, lane l: the record of geom 64 p + l into LDS, and whether its bounding sphere reaches the tile's frustum; the pass's masks of
// candidates and of opaque drawn geoms (the shadow rays' occluders)
__device__ __forceinline__ void scene_pass(const SceneArgs& sa, float* rec, int p, int lane, int f, int x0, int y0, V3 right, V3 up, V3 fwd, V3 light,
                                           unsigned long long& cand_mask, unsigned long long& occl_mask) {
  const RenderArgs& a = sa.r;
  const int NG = a.G + sa.M;
  const int g = p * PASS + lane;
  bool occl = false, cand = false;
  if (g < NG) {
    const bool dyn = g >= a.G;
    const size_t row = dyn ? (size_t)f * sa.M + (g - a.G) : (size_t)g;                  // of the type / size / rgba tables
    const size_t pose = dyn ? row : (size_t)f * a.G + g;
    const float* P = (dyn ? sa.dpos : a.pos) + pose * 3;
    const float* R = (dyn ? sa.dmat : a.mat) + pose * 9;
    const float* S = (dyn ? sa.dsize : a.size) + row * 3;
    const int type = (dyn ? sa.dtype : a.type)[row];
    const float alpha = (dyn ? sa.drgba : a.rgba)[row * 4 + 3];
    float* r = rec + g * REC;
    const V3 pp{P[0], P[1], P[2]}, s{S[0], S[1], S[2]};
    float Rl[9];
    for (int k = 0; k < 9; k++) Rl[k] = R[k];
    const V3 o = to_local(Rl, V3{-pp.x, -pp.y, -pp.z}), ll = to_local(Rl, light);
    r[0] = o.x; r[1] = o.y; r[2] = o.z;
    for (int k = 0; k < 9; k++) r[3 + k] = Rl[k];
    r[12] = s.x; r[13] = s.y; r[14] = s.z;
    r[15] = ll.x; r[16] = ll.y; r[17] = ll.z;
    r[18] = (float)type;
    r[19] = alpha;
    const bool drawn = alpha != 0.f;
    occl = drawn && !(alpha > 0.f && alpha < 1.f);
    cand = drawn;
    if (drawn && a.cull && type != G_PLANE) {
      const float cx = dot3(right, pp), cy = dot3(up, pp), cz = dot3(fwd, pp);
      const float br = type == G_CONE ? sqrtf(s.x * s.x + s.y * s.y) : bound_radius(type, s);
      const float m = 1.01f * br + 1e-4f * (1.f + fabsf(cx) + fabsf(cy) + fabsf(cz));
      const float kx = a.tan_half * a.aspect, ky = a.tan_half;
      const float xl = kx * (2.f * (float)x0 / (float)a.W - 1.f), xr = kx * (2.f * (float)(x0 + 8) / (float)a.W - 1.f);
      const float yt = -ky * (2.f * (float)y0 / (float)a.H - 1.f), yb = -ky * (2.f * (float)(y0 + 8) / (float)a.H - 1.f);
      cand = (cx - xl * cz >= -m * sqrtf(1.f + xl * xl)) && (xr * cz - cx >= -m * sqrtf(1.f + xr * xr)) &&
             (cy - yb * cz >= -m * sqrtf(1.f + yb * yb)) && (yt * cz - cy >= -m * sqrtf(1.f + yt * yt));
    }
  }
  occl_mask = __ballot(occl);
  cand_mask = __ballot(cand);
}

template <int PASSES>
__global__ void __launch_bounds__(64) scene_kernel(SceneArgs sa) {
  __shared__ float rec[PASSES * PASS * REC];      // record as render_kernel's; [19] = alpha
  __shared__ uint32_t tile_rgb[48];
  LHW_LDS_POISON(rec);
  LHW_LDS_POISON(tile_rgb);
  const RenderArgs& a = sa.r;
  const int lane = threadIdx.x;
  const int f = blockIdx.x / a.tiles, tile = blockIdx.x - f * a.tiles;
  const int x0 = (tile % a.tiles_x) * 8, y0 = (tile / a.tiles_x) * 8;
  const float* cam = a.cam + (size_t)f * 12;
  const V3 right{cam[0], cam[1], cam[2]}, up{cam[3], cam[4], cam[5]}, fwd{cam[6], cam[7], cam[8]};
  const V3 light{a.light[0], a.light[1], a.light[2]};
  const int NG = a.G + sa.M;

  unsigned long long c0 = 0, c1 = 0, c2 = 0, c3 = 0, o0 = 0, o1 = 0, o2 = 0, o3 = 0;
  scene_pass(sa, rec, 0, lane, f, x0, y0, right, up, fwd, light, c0, o0);
  if (PASSES > 1) scene_pass(sa, rec, 1, lane, f, x0, y0, right, up, fwd, light, c1, o1);
  if (PASSES > 2) scene_pass(sa, rec, 2, lane, f, x0, y0, right, up, fwd, light, c2, o2);
  if (PASSES > 3) scene_pass(sa, rec, 3, lane, f, x0, y0, right, up, fwd, light, c3, o3);
  __syncthreads();
  const int passes = (NG + PASS - 1) / PASS;

  // ---- primary rays: lane = pixel (lane % 8, lane / 8) of the tile
  const int px = x0 + (lane & 7), py = y0 + (lane >> 3);
  const float sx = a.tan_half * a.aspect * (2.f * ((float)px + 0.5f) / (float)a.W - 1.f);
  const float sy = -a.tan_half * (2.f * ((float)py + 0.5f) / (float)a.H - 1.f);
  V3 d{fwd.x + sx * right.x + sy * up.x, fwd.y + sx * right.y + sy * up.y, fwd.z + sx * right.z + sy * up.z};
  {
    const float inv = 1.f / sqrtf(dot3(d, d));
    d = V3{d.x * inv, d.y * inv, d.z * inv};
  }
  float best = INFINITY;
  int best_g = -1, best_part = 0;
  float lt[LAYERS];      // the nearest translucent surface points, ascending
  int lh[LAYERS];        // their geom * 8 + part
#pragma unroll
  for (int k = 0; k < LAYERS; k++) { lt[k] = INFINITY; lh[k] = -1; }
  for (int p = 0; p < passes; p++) {
    unsigned long long mask = pick(p, c0, c1, c2, c3);
    while (mask) {
      const int g = p * PASS + __ffsll(mask) - 1;
      mask &= mask - 1;
      const float* r = rec + g * REC;
      const float alpha = r[19];
      float t;
      int part;
      if (intersect_scene((int)r[18], V3{r[12], r[13], r[14]}, V3{r[0], r[1], r[2]}, to_local(r + 3, d), t, part)) {
        if (alpha > 0.f && alpha < 1.f) {
          int h = g * 8 + part;
#pragma unroll
          for (int k = 0; k < LAYERS; k++)
            if (t < lt[k]) { const float tt = lt[k]; const int hh = lh[k]; lt[k] = t; lh[k] = h; t = tt; h = hh; }
        } else if (t < best) {
          best = t; best_g = g; best_part = part;
        }
      }
    }
  }

  // ---- shading of the opaque surface
  V3 col{a.bg[0], a.bg[1], a.bg[2]};
  V3 so{0.f, 0.f, 0.f};      // shadow ray origin (world, relative to the camera)
  bool want_shadow = false;
  float ndl = 0.f;
  if (best_g >= 0) {
    const float* r = rec + best_g * REC;
    const int type = (int)r[18];
    const V3 s{r[12], r[13], r[14]}, o{r[0], r[1], r[2]}, dl = to_local(r + 3, d);
    const V3 pl{o.x + best * dl.x, o.y + best * dl.y, o.z + best * dl.z};
    const V3 n = to_world(r + 3, normal_scene(type, s, pl, best_part, o));
    ndl = fmaxf(0.f, dot3(n, light));
    const V3 hw{best * d.x, best * d.y, best * d.z};
    const float* c = best_g >= a.G ? sa.drgba + 4 * ((size_t)f * sa.M + (best_g - a.G)) : a.rgba + 4 * best_g;
    col = V3{c[0], c[1], c[2]};
    if (type == G_PLANE && a.checker > 0.f) {
      const int ix = (int)floorf((cam[9] + hw.x) / a.checker), iy = (int)floorf((cam[10] + hw.y) / a.checker);
      if ((ix + iy) & 1) col = V3{0.8f * col.x, 0.8f * col.y, 0.8f * col.z};
    }
    so = V3{hw.x + 1e-3f * n.x, hw.y + 1e-3f * n.y, hw.z + 1e-3f * n.z};
    want_shadow = a.shadows != 0 && ndl > 0.f;
  }
  if (a.shadows) {
    bool open = want_shadow;      // still looking for an occluder
    for (int p = 0; p < passes; p++) {
      unsigned long long sm = pick(p, o0, o1, o2, o3);
      while (sm && __any(open)) {
        const int g = p * PASS + __ffsll(sm) - 1;
        sm &= sm - 1;
        if (open) {
          const float* r = rec + g * REC;
          const V3 o{r[0], r[1], r[2]};      // o = -R^T p, so R^T (so - p) = R^T so + o
          const V3 sl = to_local(r + 3, so);
          float t;
          int part;
          if (intersect_scene((int)r[18], V3{r[12], r[13], r[14]}, V3{o.x + sl.x, o.y + sl.y, o.z + sl.z}, V3{r[15], r[16], r[17]}, t, part)) open = false;
        }
      }
    }
    if (want_shadow && !open) ndl = 0.f;
  }
  if (best_g >= 0) {
    const float sh = a.ambient + a.diffuse * ndl;
    col = V3{col.x * sh, col.y * sh, col.z * sh};
  }

  // ---- the layers in front of it, front to back
  int nl = 0;
  {
    float through = 1.f;
    V3 acc{0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < LAYERS; k++) {
      if (lt[k] < best) {      // (sorted: the layers in front of the opaque surface are a prefix of the list)
        nl++;
        const int g = lh[k] >> 3;
        const float* r = rec + g * REC;
        const int type = (int)r[18];
        const V3 s{r[12], r[13], r[14]}, o{r[0], r[1], r[2]}, dl = to_local(r + 3, d);
        const V3 pl{o.x + lt[k] * dl.x, o.y + lt[k] * dl.y, o.z + lt[k] * dl.z};
        const V3 n = to_world(r + 3, normal_scene(type, s, pl, lh[k] & 7, o));
        const float* c = g >= a.G ? sa.drgba + 4 * ((size_t)f * sa.M + (g - a.G)) : a.rgba + 4 * g;
        V3 lc{c[0], c[1], c[2]};
        if (type == G_PLANE && a.checker > 0.f) {
          const int ix = (int)floorf((cam[9] + lt[k] * d.x) / a.checker), iy = (int)floorf((cam[10] + lt[k] * d.y) / a.checker);
          if ((ix + iy) & 1) lc = V3{0.8f * lc.x, 0.8f * lc.y, 0.8f * lc.z};
        }
        const float w = through * c[3] * (a.ambient + a.diffuse * fmaxf(0.f, dot3(n, light)));
        acc = V3{acc.x + w * lc.x, acc.y + w * lc.y, acc.z + w * lc.z};
        through *= 1.f - c[3];
      }
    }
    if (nl) col = V3{acc.x + through * col.x, acc.y + through * col.y, acc.z + through * col.z};
  }

  // ---- output: per-pixel words per lane, colours through LDS
  const bool inside = px < a.W && py < a.H;
  const size_t pix = ((size_t)f * a.H + py) * a.W + px;
  if (inside) {
    if (a.hit) a.hit[pix] = best_g >= 0 ? best_g * 8 + best_part : -1;
    if (a.depth) a.depth[pix] = best;
    if (sa.layers) sa.layers[pix] = nl;
    if (sa.layer_hit) sa.layer_hit[pix] = nl ? lh[0] : -1;
  }
  uint8_t* tb = reinterpret_cast<uint8_t*>(tile_rgb);
  tb[3 * lane] = to_byte(col.x); tb[3 * lane + 1] = to_byte(col.y); tb[3 * lane + 2] = to_byte(col.z);
  __syncthreads();
  const int rows = min(8, a.H - y0), cols = min(8, a.W - x0);
  uint8_t* out = a.rgb + (((size_t)f * a.H + y0) * a.W + x0) * 3;
  const size_t pitch = (size_t)a.W * 3;
  if (cols == 8 && ((uintptr_t)out & 3) == 0 && (pitch & 3) == 0) {      // a full-width tile of dword-aligned rows: six dwords per row
    if (lane < 6 * rows) {
      const int row = lane / 6, k = lane - 6 * row;
      reinterpret_cast<uint32_t*>(out + row * pitch)[k] = tile_rgb[6 * row + k];
    }
  } else {
    for (int b = lane; b < 192; b += 64) {
      const int row = b / 24, k = b - 24 * row;
      if (row < rows && k < 3 * cols) out[row * pitch + k] = tb[b];
    }
  }
}

// type / size / alpha tables of n geoms on the host: 0, or the error of the first geom that cannot be drawn
int check_geoms(const char* what, size_t n, const int32_t* type_dev, const float* size_dev, const float* rgba_dev, hipStream_t st) {
  if (!n) return LHW_OK;
  std::vector<int32_t> type(n);
  std::vector<float> size(3 * n), rgba(4 * n);
  HIPCHK(hipMemcpyAsync(type.data(), type_dev, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(size.data(), size_dev, sizeof(float) * 3 * n, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(rgba.data(), rgba_dev, sizeof(float) * 4 * n, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (size_t g = 0; g < n; g++) {
    const int t = type[g];
    if (t != G_PLANE && t != G_SPHERE && t != G_CAPSULE && t != G_ELLIPSOID && t != G_CYLINDER && t != G_BOX && t != G_CONE)
      return lhw_fail(LHW_ERR_ARG, "lhw_render_scene: %s geom %lld has type %d (plane 0, sphere 2, capsule 3, ellipsoid 4, cylinder 5, box 6, cone %d)",
                      what, (long long)g, t, (int)G_CONE);
    const int need = t == G_PLANE ? 0 : (t == G_SPHERE ? 1 : ((t == G_CAPSULE || t == G_CYLINDER || t == G_CONE) ? 2 : 3));
    for (int k = 0; k < need; k++)
      if (rgba[4 * g + 3] != 0.f && !(size[3 * g + k] > 0.f))
        return lhw_fail(LHW_ERR_ARG, "lhw_render_scene: %s geom %lld (type %d) has size[%d] = %g", what, (long long)g, t, k, (double)size[3 * g + k]);
  }
  return LHW_OK;
}

}  // namespace

extern "C" int lhw_render_scene(const LhwRenderSettings* s, int32_t G, const int32_t* geom_type_dev, const float* geom_size_dev, const float* geom_rgba_dev,
                                int32_t M, const int32_t* dyn_type_dev, const float* dyn_size_dev, const float* dyn_rgba_dev, int32_t F,
                                const float* geom_pos_dev, const float* geom_mat_dev, const float* dyn_pos_dev, const float* dyn_mat_dev, const float* cam_dev,
                                uint8_t* rgb_dev, int32_t* hit_dev, float* depth_dev, int32_t* layers_dev, int32_t* layer_hit_dev, void* stream) {
  if (!s) return lhw_fail(LHW_ERR_ARG, "lhw_render_scene: settings is NULL");
  if (G < 0 || M < 0 || F < 0) return lhw_fail(LHW_ERR_ARG, "lhw_render_scene: G = %d, M = %d, F = %d", G, M, F);
  if ((long long)G + M > LHW_RENDER_SCENE_MAX_GEOMS)
    return lhw_fail(LHW_ERR_UNSUPPORTED, "lhw_render_scene: %d static + %d dynamic geoms, one launch holds %d", G, M, LHW_RENDER_SCENE_MAX_GEOMS);
  if (s->width < 1 || s->height < 1) return lhw_fail(LHW_ERR_ARG, "lhw_render_scene: image size %d x %d", s->width, s->height);
  if (!(s->fovy_deg > 0.f && s->fovy_deg < 180.f)) return lhw_fail(LHW_ERR_ARG, "lhw_render_scene: fovy_deg = %g must lie in (0, 180)", (double)s->fovy_deg);
  if (!(s->checker_size >= 0.f)) return lhw_fail(LHW_ERR_ARG, "lhw_render_scene: checker_size = %g", (double)s->checker_size);
  if (!rgb_dev || !cam_dev || (G && (!geom_type_dev || !geom_size_dev || !geom_rgba_dev || !geom_pos_dev || !geom_mat_dev)) ||
      (M && (!dyn_type_dev || !dyn_size_dev || !dyn_rgba_dev || !dyn_pos_dev || !dyn_mat_dev)))
    return lhw_fail(LHW_ERR_ARG, "lhw_render_scene: a required buffer is NULL");
  hipStream_t st = (hipStream_t)stream;
  // the tables once on the host: a wrong type or size, static or dynamic in any frame, is refused before anything is written
  if (int rc = check_geoms("static", (size_t)G, geom_type_dev, geom_size_dev, geom_rgba_dev, st)) return rc;
  if (int rc = check_geoms("dynamic (frame-major)", (size_t)F * (size_t)M, dyn_type_dev, dyn_size_dev, dyn_rgba_dev, st)) return rc;
  if (F == 0) return LHW_OK;
  SceneArgs sa;
  RenderArgs& a = sa.r;
  a.W = s->width; a.H = s->height; a.G = G;
  a.tiles_x = (a.W + 7) / 8;
  a.tiles = a.tiles_x * ((a.H + 7) / 8);
  if ((long long)a.tiles * F > 0x7fffffffLL) return lhw_fail(LHW_ERR_ARG, "lhw_render_scene: %d frames of %d tiles exceed one launch", F, a.tiles);
  a.tan_half = (float)tan(0.5 * (double)s->fovy_deg * 3.14159265358979323846 / 180.0);
  a.aspect = (float)((double)a.W / (double)a.H);
  for (int k = 0; k < 3; k++) { a.light[k] = s->light_dir[k]; a.bg[k] = s->background[k]; }
  a.ambient = s->ambient; a.diffuse = s->diffuse; a.checker = s->checker_size;
  a.shadows = s->shadows; a.cull = s->cull;
  a.type = geom_type_dev; a.size = geom_size_dev; a.rgba = geom_rgba_dev; a.pos = geom_pos_dev; a.mat = geom_mat_dev; a.cam = cam_dev;
  a.rgb = rgb_dev; a.hit = hit_dev; a.depth = depth_dev;
  sa.M = M; sa.dtype = dyn_type_dev; sa.dsize = dyn_size_dev; sa.drgba = dyn_rgba_dev; sa.dpos = dyn_pos_dev; sa.dmat = dyn_mat_dev;
  sa.layers = layers_dev; sa.layer_hit = layer_hit_dev;
  const dim3 grid((unsigned)(a.tiles * F)), block(64);
  switch ((G + M + PASS - 1) / PASS) {      // the pass count sizes the workgroup's LDS
    case 0: case 1: hipLaunchKernelGGL(scene_kernel<1>, grid, block, 0, st, sa); break;
    case 2: hipLaunchKernelGGL(scene_kernel<2>, grid, block, 0, st, sa); break;
    case 3: hipLaunchKernelGGL(scene_kernel<3>, grid, block, 0, st, sa); break;
    default: hipLaunchKernelGGL(scene_kernel<4>, grid, block, 0, st, sa); break;
  }
  HIPCHK(hipGetLastError());
  return LHW_OK;
}
