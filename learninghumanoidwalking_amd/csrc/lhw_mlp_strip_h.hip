// LDS-resident strip kernels of the 3-layer MLPs with fp16 operands (BASELINE config 5, --fp16 / --infer-fp16): what three (forward) or two
// (backward) gemm_h_kernel launches compute for a slab of 64 rows, in ONE launch, the activations between the layers staying in LDS as fp16.
// Opt-in (lhw_ppo_debug_set_strip_fp16, LHW_STRIP_FP16=1).  Bit for bit the per-layer path: per output element ONE
// accumulator chain of v_mfma_f32_32x32x16_f16 over the 16-k groups [0, 16), [16, 32), ... in ascending order from +0, the operands rounded to
// fp16 as gemm_h_kernel rounds them while staging (weights from the float32 master copy, k beyond K zero), then + bias and max(., 0) or the
// ReLU mask in float32, then the activation rounded to fp16 as it enters the slab (and HBM).  The operand roles are the GEMM's too: the
// activation rows are the MFMA's A operand, the weights its B operand.
// The MFMA wants eight consecutive k per lane: the slabs are stored [row][k] in fp16 (rows 16 bytes longer than a power of two: the sixteen
// lanes of a ds_read_b128 group fall on the sixteen 16-byte slots of the bank row), and the weights are read from fp16 copies in the same
// operand order, made once per change of theta (mlp_strip_h_prepare): a wave's operand load is 1024 contiguous bytes.
// Hidden width 256, padded input width <= 64, outputs <= 32: the narrow float32 strips' domain (mlp_strip_supported).
#include "lhw_mlp_strip_h.h"

#include "lhw_internal.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

#define HS_H 256                 // hidden width the kernels are compiled for
#define HS_ROWS 64               // rows per slab: two 32-row MFMA tiles
#define HS_LD (HS_H + 8)         // activation slab [HS_ROWS][HS_LD] halves: 33 KB
#define HS_XK 64                 // capacity of the input slab (padded input width of the first layer)
#define HS_XLD (HS_XK + 8)
#define HS_YK 32                 // capacity of the dy slab (outputs of the last layer)
#define HS_YLD (HS_YK + 8)
#define HS_THR 256               // four waves: wave w owns columns [64 w, 64 w + 64) of a hidden layer, all 64 rows (2 x 2 MFMA tiles)

// The weights as the kernels read them: fp16 copies in the MFMA's B-operand order.  Block (g, n) of a matrix with N columns holds the sixteen k of
// group g for output column n, [k half = lane / 32][8]: the 64 lanes of a wave (column n0 + lane % 32, k half lane / 32) read 1024 contiguous bytes
// per operand, one 16-byte vector each.  Five regions per network, zero where k or n is beyond the matrix (no guards in the K loops):
//   W1 [4 groups][256] from W1[n][k] (k < Dp)      W2 [16][256] from W2[n][k]      W3 [16][32] from W3[n][k] (n < O)          -- forward
//   W3T [2][256] from W3[k][n] (k < O)             W2T [16][256] from W2[k][n]                                                -- backward
#define HS_W1 0
#define HS_W2 (HS_W1 + 4 * HS_H * 16)
#define HS_W3 (HS_W2 + 16 * HS_H * 16)
#define HS_W3T (HS_W3 + 16 * 32 * 16)
#define HS_W2T (HS_W3T + 2 * HS_H * 16)
static_assert(HS_W2T + 16 * HS_H * 16 == MLP_STRIP_H_WH_HALVES, "the five regions");
__global__ void __launch_bounds__(256) mlp_strip_h_prepare_kernel(const float* __restrict__ w1, const float* __restrict__ w2, const float* __restrict__ w3,
                                                                  int Dp, int O, _Float16* __restrict__ wh) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= MLP_STRIP_H_WH_HALVES) return;
  const int N = (i >= HS_W3 && i < HS_W3T) ? 32 : HS_H;
  const int base = i >= HS_W2T ? HS_W2T : i >= HS_W3T ? HS_W3T : i >= HS_W3 ? HS_W3 : i >= HS_W2 ? HS_W2 : HS_W1;
  const int e = i - base, k = 16 * (e / (16 * N)) + (e & 15), n = (e >> 4) % N;
  float v = 0.f;
  if (base == HS_W1) { if (k < Dp) v = w1[(size_t)n * Dp + k]; }   // (the backward test hook: Dp = 0, no W1)
  else if (base == HS_W2) v = w2[(size_t)n * HS_H + k];
  else if (base == HS_W3) { if (n < O) v = w3[(size_t)n * HS_H + k]; }
  else if (base == HS_W3T) { if (k < O) v = w3[(size_t)k * HS_H + n]; }
  else v = w2[(size_t)k * HS_H + n];
  wh[i] = (_Float16)v;
}
void mlp_strip_h_prepare(const float* w1, const float* w2, const float* w3, int Dp, int O, _Float16* wh, hipStream_t s) {
  hipLaunchKernelGGL(mlp_strip_h_prepare_kernel, dim3(MLP_STRIP_H_WH_HALVES / 256), dim3(256), 0, s, w1, w2, w3, Dp, O, wh);
}
// One layer for the calling wave: acc[i][j] = S[32 i .. + 31][0 .. 16 G) x W (columns n0 + 32 j .. + 31 of a region with N columns), one chain per
// element, the groups in ascending order.  S holds zeros in the columns beyond the layer's K.  The weights of group g + HS_PF are in flight while
// group g is multiplied.
#define HS_PF 4
template <int NI, int NJ>
__device__ __forceinline__ void hs_layer(f32x16 (&acc)[NI][NJ], const _Float16* S, int lds, const _Float16* __restrict__ W, int N, int G, int n0) {
  const int lane = threadIdx.x & 63, l31 = lane & 31, kh = lane >> 5;
#pragma unroll
  for (int i = 0; i < NI; i++)
#pragma unroll
    for (int j = 0; j < NJ; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;
  const _Float16* Wl = W + (size_t)(n0 + l31) * 16 + 8 * kh;       // this lane's vector of group 0, column tile 0
  auto load = [&](f16x8 (&b)[NJ], int g) {
#pragma unroll
    for (int j = 0; j < NJ; j++) b[j] = *reinterpret_cast<const f16x8*>(Wl + ((size_t)g * N + 32 * j) * 16);
  };
  f16x8 b[HS_PF][NJ];
#pragma unroll
  for (int p = 0; p < HS_PF; p++)
    if (p < G) load(b[p], p);
  for (int g0 = 0; g0 < G; g0 += HS_PF) {
#pragma unroll
    for (int p = 0; p < HS_PF; p++) {
      const int g = g0 + p;
      if (g < G) {
        f16x8 a[NI], cur[NJ];
#pragma unroll
        for (int j = 0; j < NJ; j++) cur[j] = b[p][j];
        if (g + HS_PF < G) load(b[p], g + HS_PF);
#pragma unroll
        for (int i = 0; i < NI; i++) a[i] = *reinterpret_cast<const f16x8*>(S + (size_t)(32 * i + l31) * lds + 16 * g + 8 * kh);
#pragma unroll
        for (int i = 0; i < NI; i++)
#pragma unroll
          for (int j = 0; j < NJ; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i], cur[j], acc[i][j], 0, 0, 0);
      }
    }
  }
}
// The GEMM's epilogue into the slab: + bias (0 without one), max(., 0), rounded to fp16.  C/D map of the 32x32 MFMA: col = lane & 31,
// row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
template <bool RELU>
__device__ __forceinline__ void hs_acc_to_slab(const f32x16 (&acc)[2][2], _Float16 (&S)[HS_ROWS][HS_LD], const float* __restrict__ bias, int n0) {
  const int lane = threadIdx.x & 63, l31 = lane & 31, kh = lane >> 5;
#pragma unroll
  for (int j = 0; j < 2; j++) {
    const int col = n0 + 32 * j + l31;
    const float b = bias ? bias[col] : 0.f;
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        float v = acc[i][j][r] + b;
        if (RELU) v = fmaxf(v, 0.f);
        S[32 * i + (r & 3) + 8 * (r >> 2) + 4 * kh][col] = (_Float16)v;
      }
  }
}
// The slab's live rows -> out [live][256] as 16-byte vectors (out may be NULL).  MASK: entries whose mask value (the stored fp16 activation
// of the forward pass) is not > 0 become +0 first, in the slab too -- the mask commutes with the rounding that has already happened.
template <bool MASK>
__device__ __forceinline__ void hs_slab_out(_Float16 (&S)[HS_ROWS][HS_LD], _Float16* __restrict__ out, const _Float16* __restrict__ mask, int live) {
  for (int v = threadIdx.x; v < HS_ROWS * (HS_H / 8); v += HS_THR) {
    const int row = v >> 5, c = (v & 31) * 8;
    if (row >= live) break;   // (rows ascend with v)
    f16x8 x = *reinterpret_cast<const f16x8*>(&S[row][c]);
    if (MASK) {
      const f16x8 m = *reinterpret_cast<const f16x8*>(mask + (size_t)row * HS_H + c);
#pragma unroll
      for (int q = 0; q < 8; q++) x[q] = (float)m[q] > 0.f ? x[q] : (_Float16)0.f;
      *reinterpret_cast<f16x8*>(&S[row][c]) = x;
    }
    if (out) *reinterpret_cast<f16x8*>(out + (size_t)row * HS_H + c) = x;
  }
}

__global__ void __launch_bounds__(HS_THR) mlp_fwd_strip_h_kernel(MlpStripFwdH a) {
  __shared__ __attribute__((aligned(16))) _Float16 Xs[HS_ROWS][HS_XLD];
  LHW_LDS_POISON(Xs);
  __shared__ __attribute__((aligned(16))) _Float16 Hs[HS_ROWS][HS_LD];
  LHW_LDS_POISON(Hs);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n0 = 64 * wave;
  const size_t r0 = (size_t)blockIdx.x * HS_ROWS;
  const int live = min(HS_ROWS, a.R - (int)r0);
  // the input slab: fp16 rows as they are, float32 rows rounded; columns >= Dp and rows >= R zero
  for (int e = tid; e < HS_ROWS * HS_XK; e += HS_THR) {
    const int row = e >> 6, c = e & 63;
    _Float16 v = (_Float16)0.f;
    if (row < live && c < a.Dp) v = a.x_h ? a.x_h[(r0 + row) * a.ldxh + c] : (_Float16)a.x[(r0 + row) * a.ldx + c];
    Xs[row][c] = v;
  }
  __syncthreads();
  f32x16 acc[2][2];
  hs_layer<2, 2>(acc, &Xs[0][0], HS_XLD, a.wh + HS_W1, HS_H, (a.Dp + 15) >> 4, n0);
  hs_acc_to_slab<true>(acc, Hs, a.b1, n0);
  __syncthreads();
  hs_slab_out<false>(Hs, a.h1_h ? a.h1_h + r0 * HS_H : nullptr, nullptr, a.h1_h ? live : 0);
  hs_layer<2, 2>(acc, &Hs[0][0], HS_LD, a.wh + HS_W2, HS_H, HS_H / 16, n0);
  __syncthreads();   // every wave has read h1: h2 takes its place
  hs_acc_to_slab<true>(acc, Hs, a.b2, n0);
  __syncthreads();
  hs_slab_out<false>(Hs, a.h2_h ? a.h2_h + r0 * HS_H : nullptr, nullptr, a.h2_h ? live : 0);
  // the read-out, float32: one 256-k chain per element (waves 0 and 1: a row tile each, one column tile of W3's O rows)
  if (wave < 2) {
    const int l31 = lane & 31, kh = lane >> 5;
    f32x16 y[1][1];
    hs_layer<1, 1>(y, &Hs[32 * wave][0], HS_LD, a.wh + HS_W3, 32, HS_H / 16, 0);
    if (l31 < a.O) {
      const float b = a.b3[l31];
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int row = 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * kh;
        if (row < live) a.y[(r0 + row) * a.Op + l31] = y[0][0][r] + b;
      }
    }
  }
}

__global__ void __launch_bounds__(HS_THR) mlp_bwd_strip_h_kernel(MlpStripBwdH a) {
  __shared__ __attribute__((aligned(16))) _Float16 Ys[HS_ROWS][HS_YLD];
  LHW_LDS_POISON(Ys);
  __shared__ __attribute__((aligned(16))) _Float16 Hs[HS_ROWS][HS_LD];
  LHW_LDS_POISON(Hs);
  const int tid = threadIdx.x, wave = tid >> 6, n0 = 64 * wave;
  const size_t r0 = (size_t)blockIdx.x * HS_ROWS;
  const int live = min(HS_ROWS, a.R - (int)r0);
  // the dy slab: float32 rows rounded; columns >= O and rows >= R zero
  for (int e = tid; e < HS_ROWS * HS_YK; e += HS_THR) {
    const int row = e >> 5, c = e & 31;
    Ys[row][c] = (row < live && c < a.O) ? (_Float16)a.dy[(r0 + row) * a.Op + c] : (_Float16)0.f;
  }
  __syncthreads();
  f32x16 acc[2][2];
  // dh2 = (dy W3) * (h2 > 0): K = O, one or two 16-k groups
  hs_layer<2, 2>(acc, &Ys[0][0], HS_YLD, a.wh + HS_W3T, HS_H, (a.O + 15) >> 4, n0);
  hs_acc_to_slab<false>(acc, Hs, nullptr, n0);
  __syncthreads();
  hs_slab_out<true>(Hs, a.dh2_h + r0 * HS_H, a.h2_h + r0 * HS_H, live);
  __syncthreads();   // the masked dh2 is the next layer's operand
  // dh1 = (dh2 W2) * (h1 > 0)
  hs_layer<2, 2>(acc, &Hs[0][0], HS_LD, a.wh + HS_W2T, HS_H, HS_H / 16, n0);
  __syncthreads();   // every wave has read dh2: dh1 takes its place
  hs_acc_to_slab<false>(acc, Hs, nullptr, n0);
  __syncthreads();
  hs_slab_out<true>(Hs, a.dh1_h + r0 * HS_H, a.h1_h + r0 * HS_H, live);
}

bool mlp_strip_h_supported(int H, int Dp, int O, int Op) { return H == HS_H && Dp > 0 && Dp <= HS_XK && (Dp & 3) == 0 && O > 0 && O <= HS_YK && Op >= O; }
void mlp_strip_forward_h(const MlpStripFwdH& a, hipStream_t s) {
  hipLaunchKernelGGL(mlp_fwd_strip_h_kernel, dim3((a.R + HS_ROWS - 1) / HS_ROWS), dim3(HS_THR), 0, s, a);
}
void mlp_strip_backward_h(const MlpStripBwdH& a, hipStream_t s) {
  hipLaunchKernelGGL(mlp_bwd_strip_h_kernel, dim3((a.R + HS_ROWS - 1) / HS_ROWS), dim3(HS_THR), 0, s, a);
}

// ------------------------------------------------------------------------------------------- test hooks (include/lhw.h)
static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
extern "C" int lhw_debug_mlp_strip_forward_h(int32_t H, int32_t Dp, int32_t O, int32_t Op, const float* w1, const float* b1, const float* w2,
                                             const float* b2, const float* w3, const float* b3, const void* x, int32_t ldx, int32_t x_half,
                                             int32_t R, void* h1_h, void* h2_h, float* y, void* wh_scratch, void* stream) {
  if (!w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !x || !y || !wh_scratch || R <= 0) return lhw_fail(LHW_ERR_ARG, "lhw_debug_mlp_strip_forward_h: bad argument");
  if (!mlp_strip_h_supported(H, Dp, O, Op)) return lhw_fail(LHW_ERR_UNSUPPORTED, "fp16 strip kernels: hidden 256, Dp <= 64 (a multiple of 4), O <= 32");
  if (ldx < Dp || !aligned16(wh_scratch) || !aligned16(h1_h) || !aligned16(h2_h))
    return lhw_fail(LHW_ERR_ARG, "lhw_debug_mlp_strip_forward_h: ldx < Dp, or scratch / activations not 16-byte aligned");
  mlp_strip_h_prepare(w1, w2, w3, Dp, O, (_Float16*)wh_scratch, (hipStream_t)stream);
  MlpStripFwdH a{(const _Float16*)wh_scratch, b1, b2, b3, x_half ? nullptr : (const float*)x, ldx, x_half ? (const _Float16*)x : nullptr, ldx, Dp, O, Op, R,
                 (_Float16*)h1_h, (_Float16*)h2_h, y};
  mlp_strip_forward_h(a, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return LHW_OK;
}
extern "C" int lhw_debug_mlp_strip_backward_h(int32_t H, int32_t O, int32_t Op, const float* w2, const float* w3, const float* dy, int32_t R,
                                              const void* h1_h, const void* h2_h, void* dh2_h, void* dh1_h, void* wh_scratch, void* stream) {
  if (!w2 || !w3 || !dy || !h1_h || !h2_h || !dh2_h || !dh1_h || !wh_scratch || R <= 0) return lhw_fail(LHW_ERR_ARG, "lhw_debug_mlp_strip_backward_h: bad argument");
  if (!mlp_strip_h_supported(H, 4, O, Op)) return lhw_fail(LHW_ERR_UNSUPPORTED, "fp16 strip kernels: hidden 256, O <= 32");
  if (!aligned16(wh_scratch) || !aligned16(h1_h) || !aligned16(h2_h) || !aligned16(dh2_h) || !aligned16(dh1_h))
    return lhw_fail(LHW_ERR_ARG, "lhw_debug_mlp_strip_backward_h: scratch / activations not 16-byte aligned");
  mlp_strip_h_prepare(nullptr, w2, w3, 0, O, (_Float16*)wh_scratch, (hipStream_t)stream);
  MlpStripBwdH a{(const _Float16*)wh_scratch, dy, (const _Float16*)h1_h, (const _Float16*)h2_h, O, Op, R, (_Float16*)dh2_h, (_Float16*)dh1_h};
  mlp_strip_backward_h(a, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return LHW_OK;
}
