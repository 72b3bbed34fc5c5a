// The dense kernels of the PPO update: one MFMA GEMM in three operand layouts (float32 and fp16 operands), the ordered reductions of
// its split-K partials, and the two K-streaming weight-gradient kernels.  lhw_gemm.h is what the learners call.
// The float32 layers run on the gfx950 f32-input MFMA (v_mfma_f32_32x32x2_f32): bit-for-bit an fmaf chain, so results differ from ATen only by
// summation order.  GEMM design (one kernel, three operand layouts): 64x64 output tile per 256-thread workgroup,
// 4 waves in a 2x2 grid of 32x32 MFMA blocks, K staged through LDS 16 at a time, K-major LDS
// tiles so the one-float-per-lane MFMA operands are conflict-free ds_read_b32; global loads are
// 16-byte vectors, register-prefetched one tile ahead.  Epilogues fuse bias+ReLU (forward),
// ReLU-mask (backward-data), column sums (bias gradients) and split-K atomic accumulation
// (backward-weight, where the contraction runs over the minibatch).
#include "lhw_gemm.h"

#include <algorithm>
#include <cstdlib>

#include "lhw_internal.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define BM 64
#define BN 64
#define BK 16
#define LDS_LD (64 + 4)

// C = op(A) op(B) on v_mfma_f32_32x32x2_f32.  Block = 4 waves (2 x 2), each wave owns WT x WT MFMA tiles of 32 x 32:
// block tile 64 x 64 (WT = 1) or 128 x 128 (WT = 2; one LDS operand read per MFMA instead of two).  K advances in steps of
// BK = 16 through double-buffered LDS tiles: the global loads of step k+1 are in flight while step k is multiplied and there
// is one barrier per step.
// A_KC: A is stored [M][K] (K contiguous); else A is stored [K][M] (M contiguous) i.e. we multiply by its transpose.
// B_KC: B is stored [N][K] (K contiguous); else B is stored [K][N].
template <bool A_KC, bool B_KC, int WT>
__global__ void __launch_bounds__(256) gemm_f32_kernel(GemmArgs g) {
  constexpr int TM = 64 * WT, LD = TM + 4;
  __shared__ float As[2][BK][LD];
  LHW_LDS_POISON(As);
  __shared__ float Bs[2][BK][LD];
  LHW_LDS_POISON(Bs);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  // XCD-aware block order.  Workgroups are dealt round-robin to the 8 XCDs, each with its own L2, so XCD x takes the contiguous
  // range [x * per, (x + 1) * per) of the order (n tile fastest, then m tile, then k slice): the blocks that share an A tile
  // (forward / activation-gradient GEMMs: the n tiles of one m tile) or a k slice of both operands (weight-gradient GEMMs: all
  // tiles of the slice) run back to back on ONE L2 instead of being spread over all eight.
  const int per = (int)gridDim.x >> 3, v = ((int)blockIdx.x & 7) * per + ((int)blockIdx.x >> 3);
  if (v >= g.tiles_m * g.tiles_n * g.slices) return;
  const int tn = v % g.tiles_n, tm = (v / g.tiles_n) % g.tiles_m, bz = v / (g.tiles_n * g.tiles_m);
  const int m0 = tm * TM, n0 = tn * TM;
  const int kbeg = bz * g.k_chunk;
  const int kend = min(g.K, kbeg + g.k_chunk);
  f32x16 acc[WT][WT];
#pragma unroll
  for (int i = 0; i < WT; i++)
#pragma unroll
    for (int j = 0; j < WT; j++)
      for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;

  // operand staging: KC layout -> 4 / WT threads per row, each 4 * WT consecutive k; else 16 threads per k, each 4 * WT rows
  float4 ra[WT], rb[WT];
  auto load_tile = [&](float4 (&r)[WT], const float* __restrict__ P, int ld, bool kc, int x0, int X, int k0) {
#pragma unroll
    for (int q = 0; q < WT; q++) {
      r[q] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (kc) {
        const int row = x0 + tid / (4 / WT), k = k0 + (tid % (4 / WT)) * 4 * WT + 4 * q;
        if (row < X && k < kend) {
          r[q] = *reinterpret_cast<const float4*>(P + (size_t)row * ld + k);
          if (k + 1 >= kend) r[q].y = 0.f;
          if (k + 2 >= kend) r[q].z = 0.f;
          if (k + 3 >= kend) r[q].w = 0.f;
        }
      } else {
        const int k = k0 + (tid >> 4), x = x0 + (tid & 15) * 4 * WT + 4 * q;
        if (k < kend && x < X) {
          r[q] = *reinterpret_cast<const float4*>(P + (size_t)k * ld + x);
          if (x + 1 >= X) r[q].y = 0.f;
          if (x + 2 >= X) r[q].z = 0.f;
          if (x + 3 >= X) r[q].w = 0.f;
        }
      }
    }
  };
  auto store_tile = [&](float (&T)[BK][LD], const float4 (&r)[WT], bool kc) {
#pragma unroll
    for (int q = 0; q < WT; q++) {
      if (kc) {
        const int row = tid / (4 / WT), kq = (tid % (4 / WT)) * 4 * WT + 4 * q;
        T[kq + 0][row] = r[q].x; T[kq + 1][row] = r[q].y; T[kq + 2][row] = r[q].z; T[kq + 3][row] = r[q].w;
      } else {
        const int k = tid >> 4, xq = (tid & 15) * 4 * WT + 4 * q;
        *reinterpret_cast<float4*>(&T[k][xq]) = r[q];
      }
    }
  };

  const bool want_colsum = !A_KC && g.colsum != nullptr && tn == 0;
  float cs = 0.f;   // thread (m = tid % TM, k group = tid / TM): running sum of its A-tile entries
  int cur = 0;
  if (kbeg < kend) {
    load_tile(ra, g.A, g.lda, A_KC, m0, g.M, kbeg);
    load_tile(rb, g.B, g.ldb, B_KC, n0, g.N, kbeg);
    store_tile(As[0], ra, A_KC);
    store_tile(Bs[0], rb, B_KC);
  }
  __syncthreads();
  for (int k0 = kbeg; k0 < kend; k0 += BK) {
    const bool more = k0 + BK < kend;
    if (more) {
      load_tile(ra, g.A, g.lda, A_KC, m0, g.M, k0 + BK);
      load_tile(rb, g.B, g.ldb, B_KC, n0, g.N, k0 + BK);
    }
    const int l31 = lane & 31, kh = lane >> 5;
#pragma unroll
    for (int kk = 0; kk < BK / 2; kk++) {
      float a[WT], b[WT];
#pragma unroll
      for (int i = 0; i < WT; i++) a[i] = As[cur][kk * 2 + kh][(wm * WT + i) * 32 + l31];
#pragma unroll
      for (int j = 0; j < WT; j++) b[j] = Bs[cur][kk * 2 + kh][(wn * WT + j) * 32 + l31];
#pragma unroll
      for (int i = 0; i < WT; i++)
#pragma unroll
        for (int j = 0; j < WT; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    if (want_colsum) {
      constexpr int KG = BK * TM / 256;   // k rows per thread
      const int m = tid % TM, kg = tid / TM;
#pragma unroll
      for (int q = 0; q < KG; q++) cs += As[cur][kg * KG + q][m];
    }
    if (more) {
      store_tile(As[cur ^ 1], ra, A_KC);
      store_tile(Bs[cur ^ 1], rb, B_KC);
    }
    __syncthreads();
    cur ^= 1;
  }

  // epilogue; C/D map of the 32x32 MFMA: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
  float* part = g.part ? g.part + (size_t)bz * g.M * g.N : nullptr;
#pragma unroll
  for (int j = 0; j < WT; j++) {
    const int col = n0 + (wn * WT + j) * 32 + (lane & 31);
    const float bias = (g.bias && col < g.N) ? g.bias[col] : 0.f;
#pragma unroll
    for (int i = 0; i < WT; i++) {
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int row = m0 + (wm * WT + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (row < g.M && col < g.N) {
          float v = acc[i][j][r] + bias;
          if (g.relu) v = fmaxf(v, 0.f);
          if (g.mask) v = g.mask[(size_t)row * g.ldmask + col] > 0.f ? v : 0.f;
          if (part) part[(size_t)row * g.N + col] = v;
          else g.C[(size_t)row * g.ldc + col] = v;
        }
      }
    }
  }
  if (want_colsum) {   // combine the k groups in a fixed order (the tiles are idle now: the loop ended with a barrier)
    constexpr int NG = 256 / TM;
    float* red = &As[0][0][0];
    red[tid] = cs;
    __syncthreads();
    if (tid < TM && m0 + tid < g.M) {
      float s = red[tid];
#pragma unroll
      for (int q = 1; q < NG; q++) s += red[q * TM + tid];
      g.colsum[(size_t)bz * g.M + m0 + tid] = s;
    }
  }
}

// Half-precision GEMM (BASELINE config 5, "fp16 actor/critic on CDNA4"): the block order, epilogues, split-K and fused column sums of
// gemm_f32_kernel on gfx950's v_mfma_f32_32x32x16_f16 with float32 accumulation.  Round 6: the operands may LIVE in fp16 in HBM
// (a_half / b_half: the update's activations x, h1, h2 and back-propagated gradients dh2, dh1 -- written as fp16 by the GEMM that
// produces them, c_half) and are then loaded as 16-byte f16x8 vectors with no conversion; operands stored as float32 (the master weights,
// the loss gradients) are rounded while they are staged, as every operand was through round 5.  K advances 32 per step (two MFMAs per
// wave and barrier instead of one per 16-k step).  Bias / ReLU / mask in float32; outputs float32 or fp16; split-K partials float32.
// Used by the rollout inference with fp16 operands (lhw_ppo_set_inference_dtype) and by every GEMM of the --fp16 update.
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
#define HBK 32
#define HLD (HBK + 8)      // tile rows 80 bytes apart: 16-byte aligned operand reads, conflict-free across the 32 rows of a wave's read
template <bool A_KC, bool B_KC>
__global__ void __launch_bounds__(256) gemm_h_kernel(GemmArgs g) {
  __shared__ __attribute__((aligned(16))) _Float16 Ah[2][BM][HLD];
  LHW_LDS_POISON(Ah);
  __shared__ __attribute__((aligned(16))) _Float16 Bh[2][BN][HLD];
  LHW_LDS_POISON(Bh);
  __shared__ float red[256];
  LHW_LDS_POISON(red);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  const int per = (int)gridDim.x >> 3, v = ((int)blockIdx.x & 7) * per + ((int)blockIdx.x >> 3);   // XCD-aware order (gemm_f32_kernel)
  if (v >= g.tiles_m * g.tiles_n * g.slices) return;
  const int tn = v % g.tiles_n, tm = (v / g.tiles_n) % g.tiles_m, bz = v / (g.tiles_n * g.tiles_m);
  const int m0 = tm * BM, n0 = tn * BN;
  const int kbeg = bz * g.k_chunk;
  const int kend = min(g.K, kbeg + g.k_chunk);
  f32x16 acc;
  for (int r = 0; r < 16; r++) acc[r] = 0.f;
  // staging: 8 elements per thread and operand.  KC layout ([X][K]): 4 threads per row, 8 consecutive k each; else ([K][X]): 8 threads
  // per k, 8 consecutive x each.  Elements beyond the matrix / the slice are zero.
  auto load_tile = [&](const float* __restrict__ P, int ld, bool kc, bool is_half, int x0, int X, int k0) -> f16x8 {
    f16x8 r = {0, 0, 0, 0, 0, 0, 0, 0};
    const int row = kc ? x0 + (tid >> 2) : k0 + (tid >> 3);        // index along the leading dimension
    const int col = kc ? k0 + (tid & 3) * 8 : x0 + (tid & 7) * 8;  // first of the 8 contiguous elements
    const int rlim = kc ? X : kend, clim = kc ? kend : X;
    if (row < rlim && col < clim) {
      if (is_half) {
        const _Float16* Ph = reinterpret_cast<const _Float16*>(P) + (size_t)row * ld + col;
        if (col + 8 <= clim && !(((size_t)row * ld + col) & 7)) r = *reinterpret_cast<const f16x8*>(Ph);
        else for (int j = 0; j < 8; j++) if (col + j < clim) r[j] = Ph[j];
      } else {
        const float* Pf = P + (size_t)row * ld + col;
        if (col + 8 <= clim) {
          const float4 u = *reinterpret_cast<const float4*>(Pf), w = *reinterpret_cast<const float4*>(Pf + 4);
          r = f16x8{(_Float16)u.x, (_Float16)u.y, (_Float16)u.z, (_Float16)u.w, (_Float16)w.x, (_Float16)w.y, (_Float16)w.z, (_Float16)w.w};
        } else for (int j = 0; j < 8; j++) if (col + j < clim) r[j] = (_Float16)Pf[j];
      }
    }
    return r;
  };
  auto store_tile = [&](_Float16 (&T)[BM][HLD], const f16x8& r, bool kc) {
    if (kc) *reinterpret_cast<f16x8*>(&T[tid >> 2][(tid & 3) * 8]) = r;
    else {
      const int k = tid >> 3, xq = (tid & 7) * 8;
#pragma unroll
      for (int j = 0; j < 8; j++) T[xq + j][k] = r[j];
    }
  };
  const bool want_colsum = !A_KC && g.colsum != nullptr && tn == 0;
  float cs = 0.f;
  int cur = 0;
  f16x8 ra, rb;
  if (kbeg < kend) {
    ra = load_tile(g.A, g.lda, A_KC, g.a_half != 0, m0, g.M, kbeg);
    rb = load_tile(g.B, g.ldb, B_KC, g.b_half != 0, n0, g.N, kbeg);
    store_tile(Ah[0], ra, A_KC);
    store_tile(Bh[0], rb, B_KC);
  }
  __syncthreads();
  for (int k0 = kbeg; k0 < kend; k0 += HBK) {
    const bool more = k0 + HBK < kend;
    if (more) {
      ra = load_tile(g.A, g.lda, A_KC, g.a_half != 0, m0, g.M, k0 + HBK);
      rb = load_tile(g.B, g.ldb, B_KC, g.b_half != 0, n0, g.N, k0 + HBK);
    }
    const int am = wm * 32 + (lane & 31), bn = wn * 32 + (lane & 31), kh = lane >> 5;
    // v_mfma_f32_32x32x16_f16: lane l supplies k = 8 (l / 32) .. + 7 of its row / column: one 16-byte LDS read per operand
#pragma unroll
    for (int kk = 0; kk < HBK / 16; kk++) {
      const f16x8 a = *reinterpret_cast<const f16x8*>(&Ah[cur][am][kk * 16 + kh * 8]);
      const f16x8 b = *reinterpret_cast<const f16x8*>(&Bh[cur][bn][kk * 16 + kh * 8]);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0);
    }
    if (want_colsum) {   // thread (m = tid % 64, k group = tid / 64): the rounded entries it would also have multiplied
      const int m = tid & 63, kg = tid >> 6;
#pragma unroll
      for (int q = 0; q < 8; q++) cs += (float)Ah[cur][m][kg * 8 + q];
    }
    if (more) {
      store_tile(Ah[cur ^ 1], ra, A_KC);
      store_tile(Bh[cur ^ 1], rb, B_KC);
    }
    __syncthreads();
    cur ^= 1;
  }
  const int col = n0 + wn * 32 + (lane & 31);
  const float bias = (g.bias && col < g.N) ? g.bias[col] : 0.f;
  float* part = g.part ? g.part + (size_t)bz * g.M * g.N : nullptr;
  const _Float16* maskh = reinterpret_cast<const _Float16*>(g.mask);
  _Float16* Ch = reinterpret_cast<_Float16*>(g.C);
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const int row = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    if (row < g.M && col < g.N) {
      float v2 = acc[r] + bias;
      if (g.relu) v2 = fmaxf(v2, 0.f);
      if (g.mask) {
        const bool on = g.mask_half ? (float)maskh[(size_t)row * g.ldmask + col] > 0.f : g.mask[(size_t)row * g.ldmask + col] > 0.f;
        v2 = on ? v2 : 0.f;
      }
      if (part) part[(size_t)row * g.N + col] = v2;
      else if (g.c_half) Ch[(size_t)row * g.ldc + col] = (_Float16)v2;
      else g.C[(size_t)row * g.ldc + col] = v2;
    }
  }
  if (want_colsum) {
    red[tid] = cs;
    __syncthreads();
    if (tid < 64 && m0 + tid < g.M) g.colsum[(size_t)bz * g.M + m0 + tid] = ((red[tid] + red[64 + tid]) + red[128 + tid]) + red[192 + tid];
  }
}

// out[row*ldc + col] += sum over slices (in slice order) of part[z][row*N + col]: deterministic split-K reduction
__global__ void __launch_bounds__(256) reduce_slices_kernel(const float* __restrict__ part, int nslices, int M, int N, float* __restrict__ out, int ldc) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M * N) return;
  float s = 0.f;
  for (int z = 0; z < nslices; z++) s += part[(size_t)z * M * N + i];
  const int row = i / N, col = i - row * N;
  out[(size_t)row * ldc + col] += s;
}

// Deterministic column sums, two stages.  Stage 1: block (col tile, row chunk) sums its rows of 64 columns (4 strided
// row groups combined in a fixed order) into part[chunk][col].  Stage 2: out[col] += sum over chunks in chunk order.
__global__ void __launch_bounds__(256) colsum_det_kernel(const float* __restrict__ X, int rows, int ld, int ncols, float* __restrict__ part) {
  __shared__ float red[4][64];
  LHW_LDS_POISON(red);
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), g = threadIdx.x >> 6;
  const int per = (rows + COLSUM_CHUNKS - 1) / COLSUM_CHUNKS, r0 = blockIdx.y * per, r1 = min(rows, r0 + per);
  float s = 0.f;
  if (c < ncols)
    for (int r = r0 + g; r < r1; r += 4) s += X[(size_t)r * ld + c];
  red[g][threadIdx.x & 63] = s;
  __syncthreads();
  if (g == 0 && c < ncols) part[(size_t)blockIdx.y * ncols + c] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}
__global__ void __launch_bounds__(256) colsum_final_kernel(const float* __restrict__ part, int ncols, float* __restrict__ out) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncols) return;
  float s = 0.f;
  for (int k = 0; k < COLSUM_CHUNKS; k++) s += part[(size_t)k * ncols + c];
  out[c] += s;
}

__global__ void __launch_bounds__(256) reduce_segments_kernel(SegList L) {
  // block = 64 consecutive elements of one segment x 4 slice ranges; the four partial sums are combined in a fixed order
  __shared__ float red[4][64];
  LHW_LDS_POISON(red);
  const int e0 = blockIdx.x * 64;
  int k = 0;
  while (e0 >= L.first[k + 1]) k++;
  const Seg sg = L.s[k];
  const int e = e0 - L.first[k] + (threadIdx.x & 63), q = threadIdx.x >> 6;
  const int per = (sg.nslices + 3) >> 2, z0 = q * per, z1 = min(sg.nslices, z0 + per);
  float s = 0.f;
  if (e < sg.count) {
#pragma unroll 8
    for (int z = z0; z < z1; z++) s += sg.part[(size_t)z * sg.count + e];
  }
  red[q][threadIdx.x & 63] = s;
  __syncthreads();
  if (q == 0 && e < sg.count) {
    const int t = threadIdx.x;
    const float tot = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
    const int row = e / sg.N, col = e - row * sg.N;
    sg.dst[(size_t)row * sg.ldc + col] += tot * L.scale;
  }
}
void seg_add(SegList& L, const float* part, float* dst, int nslices, int M, int N, int ldc) {
  Seg& s = L.s[L.n];
  s.part = part; s.dst = dst; s.nslices = nslices; s.count = M * N; s.N = N; s.ldc = ldc;
  if (L.n == 0) L.first[0] = 0;
  L.first[L.n + 1] = L.first[L.n] + (M * N + 63) / 64 * 64;   // (a block never straddles two segments)
  L.n++;
}
void launch_reduce_segments(const SegList& L, hipStream_t s) {
  if (L.n == 0) return;
  hipLaunchKernelGGL(reduce_segments_kernel, dim3(L.first[L.n] / 64), dim3(256), 0, s, L);
}

// The two SKINNY weight gradients of one network in one K-streaming launch (round 5):
//   dW1 [H][Dp] = dh1^T x,  db1 = colsum(dh1),   dW3 [O][H] = dy^T h2,  db3 = colsum(dy)        (H = 256, Dp <= 64, O <= 32)
// Both contract over the minibatch rows and are bound by streaming one [R][256] activation array each (dh1, h2); as two 64 x 64-tile
// split-K GEMMs with 128-row slices they ran at 1.3 TB/s (23 + 26 us per 32768 rows: a thousand short blocks, prologue and epilogue
// per 128 rows).  Here a block of 8 waves takes `kc` consecutive rows and keeps BOTH products' whole outputs in registers -- wave w
// owns rows 32 w .. 32 w + 31 of dW1 (two 32 x 32 MFMA tiles across the padded Dp) and columns 32 w .. + 31 of dW3 (one tile) --
// while the rows stream through double-buffered LDS tiles in their row-major order ([r][256]: lane = column, the MFMA's operand
// layout for a product that contracts over r).  Partials per block: 256 x Dp + O x 256 + 256 + O floats, reduced in slice order by
// reduce_segments like every other weight gradient (same seed -> same bits).
#define WS_KS 16
#define WS_H 256
__global__ void __launch_bounds__(512) wgrad_skinny_kernel(WgradSkinnyArgs g) {
  __shared__ float Dh[2][WS_KS][WS_H + 4];
  LHW_LDS_POISON(Dh);
  __shared__ float Hs[2][WS_KS][WS_H + 4];
  LHW_LDS_POISON(Hs);
  __shared__ float Xs[2][WS_KS][64 + 4];
  LHW_LDS_POISON(Xs);
  __shared__ float Ys[2][WS_KS][32 + 4];
  LHW_LDS_POISON(Ys);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, kh = lane >> 5;
  const int bz = (int)blockIdx.x, kbeg = bz * g.kc, kend = min(g.R, kbeg + g.kc);
  f32x16 a1[2], a3;
  for (int r = 0; r < 16; r++) { a1[0][r] = 0.f; a1[1][r] = 0.f; a3[r] = 0.f; }
  float4 rd[2], rh[2], rx, ry;
  auto load = [&](int k0) {
#pragma unroll
    for (int q = 0; q < 2; q++) {
      const int idx = tid + 512 * q, row = idx >> 6, c4 = idx & 63, k = k0 + row;
      rd[q] = rh[q] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (k < kend) {
        rd[q] = *reinterpret_cast<const float4*>(g.dh1 + (size_t)k * WS_H + 4 * c4);
        rh[q] = *reinterpret_cast<const float4*>(g.h2 + (size_t)k * WS_H + 4 * c4);
      }
    }
    rx = ry = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tid < 256) {
      const int row = tid >> 4, c4 = tid & 15, k = k0 + row;
      if (k < kend && 4 * c4 < g.Dp) rx = *reinterpret_cast<const float4*>(g.x + (size_t)k * g.ldx + 4 * c4);   // (Dp is a multiple of 4)
    } else if (tid < 384) {
      const int row = (tid - 256) >> 3, c4 = (tid - 256) & 7, k = k0 + row;
      if (k < kend && 4 * c4 < g.Op) {
        ry = *reinterpret_cast<const float4*>(g.dy + (size_t)k * g.Op + 4 * c4);
        if (4 * c4 + 1 >= g.O) ry.y = 0.f;
        if (4 * c4 + 2 >= g.O) ry.z = 0.f;
        if (4 * c4 + 3 >= g.O) ry.w = 0.f;
        if (4 * c4 >= g.O) ry.x = 0.f;
      }
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int q = 0; q < 2; q++) {
      const int idx = tid + 512 * q, row = idx >> 6, c4 = idx & 63;
      *reinterpret_cast<float4*>(&Dh[buf][row][4 * c4]) = rd[q];
      *reinterpret_cast<float4*>(&Hs[buf][row][4 * c4]) = rh[q];
    }
    if (tid < 256) *reinterpret_cast<float4*>(&Xs[buf][tid >> 4][4 * (tid & 15)]) = rx;
    else if (tid < 384) *reinterpret_cast<float4*>(&Ys[buf][(tid - 256) >> 3][4 * ((tid - 256) & 7)]) = ry;
  };
  float cs1 = 0.f, cs3 = 0.f;   // thread (m = tid % 256, k group = tid / 256): column sum of dh1; thread t < 32: column sum of dy
  int cur = 0;
  if (kbeg < kend) { load(kbeg); store(0); }
  __syncthreads();
  for (int k0 = kbeg; k0 < kend; k0 += WS_KS) {
    const bool more = k0 + WS_KS < kend;
    if (more) load(k0 + WS_KS);
#pragma unroll
    for (int kk = 0; kk < WS_KS / 2; kk++) {
      const int k = kk * 2 + kh;
      const float ad = Dh[cur][k][32 * wave + l31], bx0 = Xs[cur][k][l31], bx1 = Xs[cur][k][32 + l31];
      const float ay = Ys[cur][k][l31], bh = Hs[cur][k][32 * wave + l31];
      a1[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(ad, bx0, a1[0], 0, 0, 0);
      a1[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(ad, bx1, a1[1], 0, 0, 0);
      a3 = __builtin_amdgcn_mfma_f32_32x32x2f32(ay, bh, a3, 0, 0, 0);
    }
    {
      const int m = tid & 255, kg = tid >> 8;
#pragma unroll
      for (int q = 0; q < WS_KS / 2; q++) cs1 += Dh[cur][kg * (WS_KS / 2) + q][m];
      if (tid < 32) {
#pragma unroll
        for (int q = 0; q < WS_KS; q++) cs3 += Ys[cur][q][tid];
      }
    }
    if (more) store(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  }
  // epilogue; C/D map of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
  float* pw1 = g.pw1 + (size_t)bz * WS_H * g.Dp;
  float* pw3 = g.pw3 + (size_t)bz * g.O * WS_H;
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const int rr = (r & 3) + 8 * (r >> 2) + 4 * kh;
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const int col = 32 * j + l31;
      if (col < g.Dp) pw1[(size_t)(32 * wave + rr) * g.Dp + col] = a1[j][r];
    }
    if (rr < g.O) pw3[(size_t)rr * WS_H + 32 * wave + l31] = a3[r];
  }
  float* red = &Dh[0][0][0];   // (the tiles are idle: the loop ended with a barrier)
  red[tid] = cs1;
  __syncthreads();
  if (tid < 256) g.pb1[(size_t)bz * WS_H + tid] = red[tid] + red[256 + tid];
  if (tid < g.O) g.pb3[(size_t)bz * g.O + tid] = cs3;
}
bool fused_skinny_on() {   // LHW_WGRAD_FUSED=0: the two split-K GEMMs instead (A/B measurements)
  static const bool on = !(getenv("LHW_WGRAD_FUSED") && atoi(getenv("LHW_WGRAD_FUSED")) == 0);
  return on;
}
int wgrad_skinny_chunk(int R) {   // rows per block: about 256 blocks per launch, at least the slice length the partial regions are sized for
  const int kc = ((R + 255) / 256 + WS_KS - 1) / WS_KS * WS_KS;
  return kc < 128 ? 128 : kc;
}
bool wgrad_skinny_supported(int H, int Dp, int O, int Op) { return H == WS_H && Dp > 0 && Dp <= 64 && (Dp & 3) == 0 && O > 0 && O <= 32 && Op >= O && Op <= 32 && (Op & 3) == 0; }
void launch_wgrad_skinny(const WgradSkinnyArgs& a, hipStream_t s) { hipLaunchKernelGGL(wgrad_skinny_kernel, dim3((a.R + a.kc - 1) / a.kc), dim3(512), 0, s, a); }

// The WIDE weight gradient dW2 [256][256] = dh2^T h1 (and db2 = colsum(dh2)) without LDS and without barriers (round 6).  Both operands
// are stored [row][256] and the product contracts over the rows, so row k of either IS the MFMA's operand layout (lane l: unit l % 32
// of row k + l / 32): a wave's load instruction fetches two 128-byte segments straight from HBM / L2, as the strip kernels load their
// weights.  Block tile 128 x 128 (four per k slice), wave tile 64 x 64 = 2 x 2 MFMA tiles: one operand load per MFMA (the LDS-staged
// 64 x 64-tile GEMM: two LDS reads per MFMA and a barrier every 16 rows, 65 us per 32768 rows = 42 % of the f32 MFMA peak).  The rows
// of chunk s + 1 are in flight while chunk s is multiplied.  XCD-aware block order: the four tiles of a k slice run on one L2.
// The bias gradient comes from the same operand registers: waves with tn == wn == 0 keep a running sum of their dh2 entries (per
// lane ascending k of one parity, the two parities added at the end: a fixed order).
struct WgradWideArgs {
  const float *A, *B;      // [K][256] each: dh2, h1
  int K, k_chunk, slices;
  float *part, *colsum;    // slice z: part + z * 256 * 256 (row-major [m][n]), colsum + z * 256
};
#define WW_H 256
// KS: rows per register buffer.  Two buffers: the loads of chunk s + 1 are issued before chunk s is multiplied, i.e. KS / 2 x 4 MFMAs
// (KS x 128 cycles when the wave has its SIMD's MFMA pipe to itself) ahead of their use.  In the update the operands come from HBM (the
// forward pass wrote h1 a few hundred MB of traffic earlier): KS = 32 (1.7 us ahead); with KS = 16 the kernel was faster than the
// LDS-staged GEMM alone on cache-warm operands and slower inside the update (profiles/r06_wgrad_wide.txt).
template <int KS>
struct WwOp { float a[KS / 2][2], b[KS / 2][2]; };
template <int KS>
__device__ __forceinline__ void ww_load(WwOp<KS>& w, const float* __restrict__ A, const float* __restrict__ B, const int k0, const int kend, const int am, const int bn) {
  const int kh = (threadIdx.x & 63) >> 5;
#pragma unroll
  for (int kk = 0; kk < KS / 2; kk++) {
    const int k = k0 + 2 * kk + kh, kc = min(k, kend - 1);
    const bool live = k < kend;
#pragma unroll
    for (int i = 0; i < 2; i++) {
      const float av = A[(size_t)kc * WW_H + am + 32 * i];
      w.a[kk][i] = live ? av : 0.f;                       // (rows beyond the slice: a zero dh2 entry, times a valid row of h1)
      w.b[kk][i] = B[(size_t)kc * WW_H + bn + 32 * i];
    }
  }
}
template <int KS>
__global__ void __launch_bounds__(256, 2) wgrad_wide_kernel(WgradWideArgs g) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, kh = lane >> 5;
  const int per = (int)gridDim.x >> 3, v = ((int)blockIdx.x & 7) * per + ((int)blockIdx.x >> 3);
  if (v >= 4 * g.slices) return;
  const int t = v & 3, tm = t >> 1, tn = t & 1, bz = v >> 2, wm = wave & 1, wn = wave >> 1;
  const int m0 = tm * 128 + wm * 64, n0 = tn * 128 + wn * 64;
  const int kbeg = bz * g.k_chunk, kend = min(g.K, kbeg + g.k_chunk);
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;
  float cs[2] = {0.f, 0.f};
  WwOp<KS> w0, w1;
  auto mul = [&](const WwOp<KS>& w) {
#pragma unroll
    for (int kk = 0; kk < KS / 2; kk++) {
#pragma unroll
      for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.a[kk][i], w.b[kk][j], acc[i][j], 0, 0, 0);
      cs[0] += w.a[kk][0]; cs[1] += w.a[kk][1];
    }
  };
  if (kbeg < kend) {
    ww_load<KS>(w0, g.A, g.B, kbeg, kend, m0 + l31, n0 + l31);
    for (int k0 = kbeg; k0 < kend; k0 += 2 * KS) {
      ww_load<KS>(w1, g.A, g.B, k0 + KS, kend, m0 + l31, n0 + l31);      // (unconditional: clamped past the end)
      __builtin_amdgcn_sched_barrier(0);
      mul(w0);
      __builtin_amdgcn_sched_barrier(0);
      ww_load<KS>(w0, g.A, g.B, k0 + 2 * KS, kend, m0 + l31, n0 + l31);
      __builtin_amdgcn_sched_barrier(0);
      if (k0 + KS < kend) mul(w1);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  // epilogue; C/D map of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
  float* part = g.part + (size_t)bz * WW_H * WW_H;
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) part[(size_t)(m0 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * kh) * WW_H + n0 + 32 * j + l31] = acc[i][j][r];
  if (g.colsum && tn == 0 && wn == 0) {
#pragma unroll
    for (int i = 0; i < 2; i++) {
      const float o = __shfl_down(cs[i], 32);
      if (kh == 0) g.colsum[(size_t)bz * WW_H + m0 + 32 * i + l31] = cs[i] + o;
    }
  }
}
bool wgrad_wide_on() {   // LHW_WGRAD_WIDE=0: the LDS-staged split-K GEMM instead (A/B measurements)
  static const bool on = !(getenv("LHW_WGRAD_WIDE") && atoi(getenv("LHW_WGRAD_WIDE")) == 0);
  return on;
}
bool wgrad_wide_supported(int H) { return H == WW_H; }
void launch_wgrad_wide(const float* A, const float* B, int K, int k_chunk, float* part, float* colsum, hipStream_t s) {
  WgradWideArgs a{A, B, K, k_chunk, (K + k_chunk - 1) / k_chunk, part, colsum};
  static const int ks = getenv("LHW_WGRAD_WIDE_KS") ? atoi(getenv("LHW_WGRAD_WIDE_KS")) : 32;   // (tuning aid)
  const dim3 grid(8 * ((4 * (size_t)a.slices + 7) / 8));
  if (ks == 16) hipLaunchKernelGGL(wgrad_wide_kernel<16>, grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL(wgrad_wide_kernel<32>, grid, dim3(256), 0, s, a);
}

template <bool A_KC, bool B_KC>
void launch_gemm(const GemmArgs& g, hipStream_t s, int defer, int wt, int half) {
  GemmArgs a = g;
  if (a.k_chunk <= 0) a.k_chunk = a.K;
  const int kstep = half ? HBK : BK;
  a.k_chunk = ((a.k_chunk + kstep - 1) / kstep) * kstep;
  const int nz = (a.K + a.k_chunk - 1) / a.k_chunk;
  static const int env_wt = getenv("LHW_GEMM_WT") ? atoi(getenv("LHW_GEMM_WT")) : 0;   // tuning aid: 1 / 2 forces the tile size
  const int force_wt = wt ? wt : env_wt;
  // 64 x 64 block tiles by default: on every shape of the update they beat the 128 x 128 variant (profiles/r02_ppo_gemm_shapes.txt:
  // at K = 256 a block's whole K loop is 16 steps, so more, smaller blocks hide the load / store phases better than fewer
  // LDS reads per MFMA help); wt = 2 (LHW_GEMM_WT=2) keeps the large tile selectable for other shapes
  const bool big = force_wt == 2;
  const int tile = (big && !half) ? 128 : 64;
  a.tiles_m = (a.M + tile - 1) / tile; a.tiles_n = (a.N + tile - 1) / tile; a.slices = nz;
  const dim3 grid(8 * (((size_t)a.tiles_m * a.tiles_n * nz + 7) / 8));
  if (half) hipLaunchKernelGGL((gemm_h_kernel<A_KC, B_KC>), grid, dim3(256), 0, s, a);
  else if (big) hipLaunchKernelGGL((gemm_f32_kernel<A_KC, B_KC, 2>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((gemm_f32_kernel<A_KC, B_KC, 1>), grid, dim3(256), 0, s, a);
  if (a.part && !defer) {  // ordered reduction of the split-K slices into the (accumulating) destination
    const int n = a.M * a.N;
    hipLaunchKernelGGL(reduce_slices_kernel, dim3((n + 255) / 256), dim3(256), 0, s, a.part, nz, a.M, a.N, a.C, a.ldc);
  }
}
template void launch_gemm<true, true>(const GemmArgs&, hipStream_t, int, int, int);
template void launch_gemm<true, false>(const GemmArgs&, hipStream_t, int, int, int);
template void launch_gemm<false, false>(const GemmArgs&, hipStream_t, int, int, int);

void colsum_det(const float* X, int rows, int ld, int ncols, float* out, float* scratch /* [COLSUM_CHUNKS][ncols] */, hipStream_t s) {
  hipLaunchKernelGGL(colsum_det_kernel, dim3((ncols + 63) / 64, COLSUM_CHUNKS), dim3(256), 0, s, X, rows, ld, ncols, scratch);
  hipLaunchKernelGGL(colsum_final_kernel, dim3((ncols + 255) / 256), dim3(256), 0, s, scratch, ncols, out);
}
// ------------------------------------------------------------------------------------------- test / tuning hooks
// Test / tuning hook: one GEMM of the update path on caller-provided device buffers (see include/lhw.h).
extern "C" int lhw_debug_gemm(int32_t a_kc, int32_t b_kc, int32_t wt, int32_t M, int32_t N, int32_t K, const float* A, int32_t lda,
                              const float* B, int32_t ldb, float* C, int32_t ldc, const float* bias, int32_t relu, const float* mask,
                              int32_t ldmask, int32_t k_chunk, float* part, float* colsum, float* colsum_out, void* stream) {
  if (!A || !B || !C || M <= 0 || N <= 0 || K <= 0 || (lda | ldb | ldc) & 3) return lhw_fail(LHW_ERR_ARG, "lhw_debug_gemm: bad argument");
  if ((colsum && (a_kc || !part || !colsum_out)) || (k_chunk > 0 && k_chunk < K && !part)) return lhw_fail(LHW_ERR_ARG, "lhw_debug_gemm: split-K needs part; colsum needs A stored [K][M]");
  hipStream_t s = (hipStream_t)stream;
  GemmArgs g{};
  g.A = A; g.lda = lda; g.B = B; g.ldb = ldb; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K; g.bias = bias; g.relu = relu;
  g.mask = mask; g.ldmask = ldmask; g.part = part; g.k_chunk = k_chunk; g.colsum = colsum;
  // wt = 16 .. 31: the fp16 GEMM; bits 0..3 of (wt - 16): A / B / C / mask are STORED as fp16 (else float32, rounded while staged)
  const int defer = part != nullptr, half = wt >= 16 && wt < 32;
  if (half) { g.a_half = (wt - 16) & 1; g.b_half = ((wt - 16) >> 1) & 1; g.c_half = ((wt - 16) >> 2) & 1; g.mask_half = ((wt - 16) >> 3) & 1; wt = 1; }
  if (a_kc && b_kc) launch_gemm<true, true>(g, s, defer, wt, half);
  else if (a_kc && !b_kc) launch_gemm<true, false>(g, s, defer, wt, half);
  else if (!a_kc && !b_kc) launch_gemm<false, false>(g, s, defer, wt, half);
  else return lhw_fail(LHW_ERR_UNSUPPORTED, "lhw_debug_gemm: A [K][M] with B [N][K] is not used by the update");
  if (part) {   // the deferred path of the update: partials (and column sums) reduced by one launch, accumulating into C / colsum_out
    const int kstep = half ? HBK : BK;
    const int kc = ((std::max(1, k_chunk > 0 ? k_chunk : K) + kstep - 1) / kstep) * kstep;
    SegList S;
    S.n = 0; S.scale = 1.f;
    seg_add(S, part, C, (K + kc - 1) / kc, M, N, ldc);
    if (colsum) seg_add(S, colsum, colsum_out, (K + kc - 1) / kc, M, 1, 1);
    launch_reduce_segments(S, s);
  }
  HIPCHK(hipGetLastError());
  return LHW_OK;
}

// Test hook: dW1 / db1 / dW3 / db3 of one network by the fused K-streaming kernel, ADDED to the outputs (scratch: slices x (256 Dp + 256 + 256 O + O) floats)
extern "C" int lhw_debug_wgrad_wide(const float* A, const float* B, int32_t K, int32_t k_chunk, float* part, float* colsum, void* stream) {
  if (!A || !B || !part || K <= 0 || k_chunk <= 0) return lhw_fail(LHW_ERR_ARG, "bad argument");
  launch_wgrad_wide(A, B, K, k_chunk, part, colsum, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? LHW_OK : lhw_fail(LHW_ERR_HIP, "wgrad_wide_kernel launch failed");
}
extern "C" int lhw_debug_wgrad_skinny(int32_t H, int32_t Dp, int32_t O, int32_t Op, const float* dh1, const float* x, int32_t ldx, const float* dy,
                                      const float* h2, int32_t R, float* dW1, float* db1, float* dW3, float* db3, float* scratch, void* stream) {
  if (!dh1 || !x || !dy || !h2 || !dW1 || !db1 || !dW3 || !db3 || !scratch || R <= 0) return lhw_fail(LHW_ERR_ARG, "lhw_debug_wgrad_skinny: bad argument");
  if (!wgrad_skinny_supported(H, Dp, O, Op) || ldx < Dp || (ldx & 3)) return lhw_fail(LHW_ERR_UNSUPPORTED, "fused skinny weight gradients: hidden 256, Dp <= 64, O <= 32");
  hipStream_t s = (hipStream_t)stream;
  const int kc = wgrad_skinny_chunk(R), ns = (R + kc - 1) / kc;
  WgradSkinnyArgs g{dh1, x, dy, h2, ldx, Dp, O, Op, R, kc, scratch, scratch + (size_t)ns * H * Dp, scratch + (size_t)ns * (H * Dp + H), scratch + (size_t)ns * (H * Dp + H + O * H)};
  launch_wgrad_skinny(g, s);
  SegList S;
  S.n = 0; S.scale = 1.f;
  seg_add(S, g.pw1, dW1, ns, H, Dp, Dp);
  seg_add(S, g.pb1, db1, ns, H, 1, 1);
  seg_add(S, g.pw3, dW3, ns, O, H, H);
  seg_add(S, g.pb3, db3, ns, O, 1, 1);
  launch_reduce_segments(S, s);
  HIPCHK(hipGetLastError());
  return LHW_OK;
}
