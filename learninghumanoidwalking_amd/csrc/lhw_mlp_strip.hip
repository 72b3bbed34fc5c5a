// LDS-resident strip kernels for the 3-layer MLPs of the PPO update (actor / critic: in -> 256 -> 256 -> out).
//
// Takes over, for one network, the layer-by-layer passes of /root/reference/rl/algos/ppo.py:299-406 (`update_actor_critic`:
// actor / critic forward, loss.backward()) that lhw_ppo.hip otherwise runs as one GEMM launch per layer with the activations
// round-tripping HBM between the launches.  A workgroup owns a SLAB of 64 rows and keeps it in LDS through all layers:
//
//   forward   x slab -> h1 = relu(x W1^T + b1) -> h2 = relu(h1 W2^T + b2) -> y = h2 W3^T + b3
//             (h1 / h2 are written to HBM once, for the backward pass, and never read back by the forward pass)
//   backward  dy slab -> dh2 = (dy W3) * (h2 > 0) -> dh1 = (dh2 W2) * (h1 > 0)
//             (dh2 / dh1 are written once, for the weight-gradient GEMMs, which contract over the minibatch rows and stay
//             split-K GEMMs in lhw_gemm.hip)
//
// The slab sits k-major in LDS (S[k][row]): that is the A-operand layout of v_mfma_f32_32x32x2_f32 (lane l: A[row = l % 32]
// [k = l / 32]), so a layer's output tile, written back column by column, IS the next layer's A operand.  The weights are the
// B operand and come straight from global memory (L2-resident, 0.3 MB per network) in [in][out] order -- for the forward pass
// from transposed copies made once per optimiser step (mlp_strip_prepare) -- so a wave's load of one k row of its 64 output
// columns is two 128-byte segments and the K loop needs no LDS staging and no barrier: 256 threads = 4 waves, wave w owns all
// 64 rows x the 64 columns 64 w .. 64 w + 63 (2 x 2 MFMA tiles: one A read and one B load feed two MFMAs each), the operands
// of K step s + 1 are in flight while step s is multiplied, and the only barriers are the two per layer around the slab
// hand-off.  70 KB of LDS per block: two blocks per CU, so one block's epilogue (the single HBM write of h / dh) overlaps the
// other's products.  The read-out layer (N <= 32) is split over K between the four waves and summed in a fixed order.
// Float32 operands and accumulation (the f32-input MFMA is an fmaf chain over ascending k), so the hidden layers are
// bit-identical to the per-layer GEMM path and the networks keep the reference's float32 semantics; only the read-out's
// summation order differs.
//
// Two sets of instantiations by the capacity XK of the input slab.  NARROW (XK = 64, padded input rows of up to 64 columns): the input slab is the
// last 64 rows of S and the read-out is the sum of partials described above.  WIDE (XK = 256 = LHW_MLP_STRIP_MAX_IN_PAD: the rows of an observation
// history, 68 .. 256 columns): the input fills S from row 0 -- it only has to live until the first layer's products are done, the accumulators
// are in registers and h1 is written behind a barrier -- so the LDS allocation and the two workgroups per CU stay; the read-out is ONE chain
// over k per row tile (fwd_readout_chain), which makes these instantiations bit-identical to the per-layer GEMM path in EVERY output, and to
// the in-wave policy step of the history rollout (policy_step_wide).  The launchers pick the instantiation by Dp.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "../../include/lhw.h"
#include "lhw_internal.h"
#include "lhw_lstm_cell.h"
#include "lhw_lstm_steps.h"
#include "lhw_policy.h"

#ifndef __HIP_EMU__
typedef float f32x16 __attribute__((ext_vector_type(16)));
#endif

#define SH 256          // hidden width the strip kernels are compiled for
#define SBK 16          // K step (one register buffer of weight operands)
#define SXK 64          // capacity of the narrow input slab (padded input width of the first layer) and of the dy slab (output width of the last)
#define SXW LHW_MLP_STRIP_MAX_IN_PAD   // capacity of the WIDE input slab (an observation history): the input fills the whole slab, S from row 0
static_assert(SXK <= SH && SXW <= SH, "the input slab is a part of the activation slab");
static_assert(SXW <= LHW_ROLLOUT_HISTORY_MAX_OBS_PAD, "every row the wide strips take has the resident history rollout (wider rows have it too: per-layer GEMMs)");
#define SKQ 32          // the read-out is summed as SH / SKQ partial products of SKQ k each, in ascending order, whatever the shape

// Shape of a workgroup: RT row tiles of 32 slab rows, NW waves, each owning CT column tiles of 32 output units (NW * CT * 32 =
// SH).  Big: 64-row slabs, 4 waves x 64 columns -- 2 x 2 MFMA tiles per wave, one slab / weight operand feeds two MFMAs each;
// 70 KB of LDS (two workgroups per CU): the update's shape.  Small: 32-row slabs, 8 waves x 32 columns -- a quarter of the
// MFMA chain per wave: the shape of rollout inference, where a few thousand rows put fewer slabs on the chip than it has CUs
// and the latency of one slab is the latency of the policy step (41 -> ~15 us).  Results are identical between the shapes (the
// hidden layers are the same fmaf chains, the read-out has the same partial sums).
template <int RT_, int CT_, int NW_>
struct StripShape {
  static constexpr int RT = RT_, CT = CT_, NW = NW_, ROWS = 32 * RT_, LD = ROWS + 4, THR = 64 * NW_;
  static_assert(NW_ * CT_ * 32 == SH, "the waves' column tiles must cover the hidden width");
};
typedef StripShape<2, 2, 4> StripBig;
typedef StripShape<1, 1, 8> StripSmall;

// -DLHW_STRIP_CLOCK (analysis builds, scripts/strip_clock.py): every wave of the first 2048 workgroups stamps the 100 MHz wall clock at
// the phase boundaries of the strip kernels; lhw_debug_strip_clock_read copies the stamps out.
#ifdef LHW_STRIP_CLOCK
#define SCLK_N 32
__device__ unsigned long long g_strip_clk[2048 * 4 * SCLK_N];
#define SCLK(k) do { if ((threadIdx.x & 63) == 0 && blockIdx.x < 2048 && (threadIdx.x >> 6) < 4) g_strip_clk[((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * SCLK_N + (k)] = wall_clock64(); } while (0)
extern "C" int lhw_debug_strip_clock_read(unsigned long long* host) {
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_strip_clk), sizeof(g_strip_clk)) == hipSuccess ? LHW_OK : LHW_ERR_HIP;
}
#else
#define SCLK(k) do { } while (0)
#endif

template <class C>
struct StripLds {
  float S[SH][C::LD];       // activation slab, k-major (Big: 69 632 B).  The input slab (x: at most XK columns, XK = SXK or SXW per
};                          // instantiation; dy: at most SXK) occupies its last XK rows until the first layer's products are done

// Which global rows a slab holds: row tile i = the 32 rows from base[i]; a tile's rows from end[i] on are not live (staged as zeros,
// never stored).  Consecutive: ROWS rows from row0.  Twins (the update's actor with mirroring): tile 0 = rows [r0, r0 + 32), tile 1 = the
// same rows of the mirrored pass, twin0 rows further on.  A row's values are fmaf chains over k: they do not depend on its slab mates.
template <class C>
struct SlabRows {
  int base[C::RT], end[C::RT];
  __device__ __forceinline__ static SlabRows consecutive(const int row0, const int R) {
    SlabRows s;
#pragma unroll
    for (int i = 0; i < C::RT; i++) { s.base[i] = row0 + 32 * i; s.end[i] = R; }
    return s;
  }
  __device__ __forceinline__ static SlabRows twins(const int r0, const int B, const int twin0) {
    SlabRows s;
#pragma unroll
    for (int i = 0; i < C::RT; i++) { s.base[i] = r0 + i * twin0; s.end[i] = B + i * twin0; }
    return s;
  }
  __device__ __forceinline__ bool full() const {
    bool f = true;
#pragma unroll
    for (int i = 0; i < C::RT; i++) f = f && base[i] + 32 <= end[i];
    return f;
  }
  // global row of slab row r, and whether it is live
  __device__ __forceinline__ int grow(const int r) const {
    int g = base[0] + r;
#pragma unroll
    for (int i = 1; i < C::RT; i++) g = r >= 32 * i ? base[i] + r - 32 * i : g;
    return g;
  }
  __device__ __forceinline__ bool live(const int r) const {
    bool v = base[0] + r < end[0];
#pragma unroll
    for (int i = 1; i < C::RT; i++) v = r >= 32 * i ? base[i] + r - 32 * i < end[i] : v;
    return v;
  }
};

template <class C>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[C::RT][C::CT]) {
#pragma unroll
  for (int i = 0; i < C::RT; i++)
#pragma unroll
    for (int j = 0; j < C::CT; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;
}

// One K step (SBK rows of k) of weights, as the MFMA wants them: lane l holds, for kk = 0 .. SBK/2, the element of row
// k0 + 2 kk + l / 32 in the wave's CT column tiles.
template <class C>
struct WOp { float v[SBK / 2][C::CT]; };

// weights of step k0 straight from global memory: stored [K][ldb] with the output unit contiguous, so one load instruction of
// the wave fetches two 128-byte segments; no LDS staging.  Rows k >= K are clamped copies of row K - 1 (the slab holds zeros
// there), so the prefetches can run past the end unconditionally.
template <class C>
__device__ __forceinline__ void wload(WOp<C>& w, const float* __restrict__ Bg, const int ldb, const int K, const int k0) {
  const int lane = threadIdx.x & 63, l31 = lane & 31, kh = lane >> 5, n0 = (threadIdx.x >> 6) * 32 * C::CT + l31;
#pragma unroll
  for (int kk = 0; kk < SBK / 2; kk++) {
    const int k = min(k0 + kk * 2 + kh, K - 1);
#pragma unroll
    for (int j = 0; j < C::CT; j++) w.v[kk][j] = Bg[(size_t)k * ldb + n0 + 32 * j];
  }
}

// acc[i][j] += (A[rows 32 i .. +32][0 .. K) * B[0 .. K)[the wave's column tile j])^T.  A is the LDS slab (k-major; rows k >= K up
// to the next multiple of SBK must hold ZEROS), B the weights (wload).  No barrier in the K loop: the waves of the block own
// disjoint output columns and share only the read-only slab.  The weights of step s + 1 are in flight while step s is
// multiplied; `w0` arrives holding the weights of step 0 (the caller issues that load early, e.g. before the previous layer's
// epilogue).
// The weights are the MFMA's A operand and the slab its B operand, so the accumulators hold the TRANSPOSED output tile: lane =
// slab row, four consecutive output units per register quad (16-byte row-major stores in the epilogue).
template <class C>
__device__ __forceinline__ void slab_mma(const float (*A)[C::LD], const int K, const float* __restrict__ Bg, const int ldb, WOp<C>& w0,
                                         f32x16 (&acc)[C::RT][C::CT]) {
  const int lane = threadIdx.x & 63, l31 = lane & 31, kh = lane >> 5;
  WOp<C> w1;
  auto mul = [&](const WOp<C>& w, int k0) {
#pragma unroll
    for (int kk = 0; kk < SBK / 2; kk++) {
      const int k = k0 + kk * 2 + kh;
      float a[C::RT];
#pragma unroll
      for (int i = 0; i < C::RT; i++) a[i] = A[k][32 * i + l31];
#pragma unroll
      for (int i = 0; i < C::RT; i++)
#pragma unroll
        for (int j = 0; j < C::CT; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.v[kk][j], a[i], acc[i][j], 0, 0, 0);
    }
  };
  // (the prefetches are unconditional, so the loop body is one straight path and a multiply waits only for its own, older,
  // loads; the scheduling barriers keep the machine scheduler from sinking a prefetch down to its first use.  Prefetching the
  // slab rows a step ahead as well measured slower: 155 vs 147 us per 65536-row forward pass)
  for (int k0 = 0; k0 < K; k0 += 2 * SBK) {
    wload<C>(w1, Bg, ldb, K, k0 + SBK);
    __builtin_amdgcn_sched_barrier(0);
    mul(w0, k0);
    __builtin_amdgcn_sched_barrier(0);
    wload<C>(w0, Bg, ldb, K, k0 + 2 * SBK);
    __builtin_amdgcn_sched_barrier(0);
    if (k0 + SBK < K) mul(w1, k0 + SBK);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// Epilogue of a 256-wide layer: v = acc (+ bias[n]) (ReLU) (masked by mask[row][n] > 0); to HBM (row-major, ld SH) and, with
// TO_SLAB, into the slab as the next layer's operand.  The accumulators hold the transposed tile (see slab_mma): lane l of tile
// (i, j) owns slab row 32 i + l % 32 and, in registers 4 g .. 4 g + 3, the output units (wave's first) + 32 j + 8 g + 4 (l / 32) +
// 0..3 -- one 16-byte store (and one 16-byte mask / bias load) per register quad.  Rows beyond R are computed (finite values
// from zero inputs) but never stored to HBM.
template <class C, bool TO_SLAB, bool FULL, int RB>
__device__ __forceinline__ void store_act_t(StripLds<C>& L, const f32x16 (&acc)[C::RT][C::CT], const float* __restrict__ bias, const bool relu,
                                            const float* __restrict__ mask, float* __restrict__ out, const SlabRows<C>& sr,
                                            unsigned* __restrict__ bits_out, const unsigned* __restrict__ bits_in, unsigned (&rb)[C::CT]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, kh = lane >> 5;
  // ReLU masks as BITS (round 6): the forward pass leaves, per thread and column tile, one word with bit (g RT + i) 4 + c set where its
  // output is positive; the backward pass -- same workgroup shape, same thread-to-element map -- reads that word instead of sixteen
  // 16-byte loads of the activations themselves (2 MB instead of 33.5 MB per layer and 32768 rows).  RB = 1 / 2: the words are written to /
  // read from rb, the thread's own registers, instead of HBM, where one kernel runs both passes (mlp_train_strip_kernel); RB = 0: rb unused.
  // (A template flag and an array REFERENCE on purpose: as optional pointers -- NULL in the plain kernels, a local array in the train kernel --
  // the words made this ROCm's clang crash in the inliner's call-graph update.  So every caller hands an array over, used or not, and the
  // kernels that keep no words declare a dummy that the optimiser drops: profiles/r08_train_strip_resources.txt -- within three VGPRs of
  // the kernels before the flag, no scratch, the same occupancy; the backward kernel now parks 6 SGPRs in VGPR lanes (106 against 104
  // SGPRs: no memory traffic, and a VGPR budget of 256 it uses 117 of).)
  unsigned wbits[C::CT];
  const bool use_bits = RB == 2 || bits_in;
#pragma unroll
  for (int j = 0; j < C::CT; j++) wbits[j] = RB == 2 ? rb[j] : (bits_in ? bits_in[((size_t)blockIdx.x * C::THR + tid) * C::CT + j] : 0u);
#pragma unroll
  for (int j = 0; j < C::CT; j++) {
    const int nb = wave * 32 * C::CT + 32 * j + 4 * kh;
    // the mask values of this column tile first, as one batch of independent loads (interleaved with the stores below they
    // would be serialised: the compiler cannot prove that `out` does not alias `mask`)
    float4 mk[C::RT][4];
#pragma unroll
    for (int i = 0; i < C::RT; i++)
#pragma unroll
      for (int g = 0; g < 4; g++) {
        mk[i][g] = make_float4(1.f, 1.f, 1.f, 1.f);
        if (mask && !use_bits && (FULL || sr.base[i] + l31 < sr.end[i])) mk[i][g] = *reinterpret_cast<const float4*>(mask + (size_t)(sr.base[i] + l31) * SH + nb + 8 * g);
      }
    unsigned ob = 0u;
#pragma unroll
    for (int g = 0; g < 4; g++) {
      const int n = nb + 8 * g;
      float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
      if (bias) bv = *reinterpret_cast<const float4*>(bias + n);
#pragma unroll
      for (int i = 0; i < C::RT; i++) {
        const int row = 32 * i + l31;
        const bool live = FULL || sr.base[i] + l31 < sr.end[i];
        float4 v = make_float4(acc[i][j][4 * g] + bv.x, acc[i][j][4 * g + 1] + bv.y, acc[i][j][4 * g + 2] + bv.z, acc[i][j][4 * g + 3] + bv.w);
        if (relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
        const int b0 = (g * C::RT + i) * 4;
        if (use_bits) {
          const unsigned w = wbits[j] >> b0;
          v.x = (live && (w & 1u)) ? v.x : 0.f; v.y = (live && (w & 2u)) ? v.y : 0.f;
          v.z = (live && (w & 4u)) ? v.z : 0.f; v.w = (live && (w & 8u)) ? v.w : 0.f;
        } else if (mask) {
          v.x = (live && mk[i][g].x > 0.f) ? v.x : 0.f; v.y = (live && mk[i][g].y > 0.f) ? v.y : 0.f;
          v.z = (live && mk[i][g].z > 0.f) ? v.z : 0.f; v.w = (live && mk[i][g].w > 0.f) ? v.w : 0.f;
        }
        if (RB == 1 || bits_out) ob |= ((v.x > 0.f ? 1u : 0u) | (v.y > 0.f ? 2u : 0u) | (v.z > 0.f ? 4u : 0u) | (v.w > 0.f ? 8u : 0u)) << b0;
        if (TO_SLAB) { L.S[n][row] = v.x; L.S[n + 1][row] = v.y; L.S[n + 2][row] = v.z; L.S[n + 3][row] = v.w; }
        if (live && out) *reinterpret_cast<float4*>(out + (size_t)(sr.base[i] + l31) * SH + n) = v;   // (out == NULL: inference, the hidden layers stay in LDS)
      }
    }
    if (bits_out) bits_out[((size_t)blockIdx.x * C::THR + tid) * C::CT + j] = ob;
    if (RB == 1) rb[j] = ob;
  }
}
template <class C, bool TO_SLAB, int RB>
__device__ __forceinline__ void store_act(StripLds<C>& L, const f32x16 (&acc)[C::RT][C::CT], const float* __restrict__ bias, const bool relu,
                                          const float* __restrict__ mask, float* __restrict__ out, const SlabRows<C>& sr,
                                          unsigned* __restrict__ bits_out, const unsigned* __restrict__ bits_in, unsigned (&rb)[C::CT]) {
  if (sr.full()) store_act_t<C, TO_SLAB, true, RB>(L, acc, bias, relu, mask, out, sr, bits_out, bits_in, rb);   // (all but the last slab: no per-row tests)
  else store_act_t<C, TO_SLAB, false, RB>(L, acc, bias, relu, mask, out, sr, bits_out, bits_in, rb);
}

// stage a [rows][K] row-major slab (row stride ld) k-major into X, zero-padded to a multiple of SBK in k and beyond R in rows
// (mean / stdv: the input is a raw observation row of in_dim entries, normalised on the way in -- the same expression as
// normalize_kernel, so the update, which normalises its minibatches there, sees the same bits)
template <class C, int XK>
__device__ __forceinline__ void stage_input(float (*X)[C::LD], const float* __restrict__ x, const int ld, const int K, const SlabRows<C>& sr,
                                            const float* __restrict__ mean = nullptr, const float* __restrict__ stdv = nullptr, const int in_dim = 0) {
  const int Kp = (K + SBK - 1) & ~(SBK - 1);
  if (!mean && !(ld & 3) && !(reinterpret_cast<size_t>(x) & 15)) {
    // 16-byte rows (the update's minibatches: x [R][Dp], dy [R][Op]): every thread issues ALL its 16-byte loads before the first LDS write
    // -- as a loop of load -> write round trips (twelve of them, dependent) this stage took 5.4 us of a 64 us forward pass
    // (profiles/r06_strip_clock.txt)
    const int k4 = Kp >> 2;
    constexpr int NQ = (C::ROWS * (XK / 4) + C::THR - 1) / C::THR;
    const float rk4 = 1.f / (float)k4;
    float4 v[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) {
      const int idx = (int)threadIdx.x + q * C::THR, r = (int)(((float)idx + 0.5f) * rk4), k = 4 * (idx - r * k4);
      v[q] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (idx < C::ROWS * k4 && k < K && sr.live(r)) {
        v[q] = *reinterpret_cast<const float4*>(x + (size_t)sr.grow(r) * ld + k);
        if (k + 1 >= K) v[q].y = 0.f;
        if (k + 2 >= K) v[q].z = 0.f;
        if (k + 3 >= K) v[q].w = 0.f;
      }
    }
#pragma unroll
    for (int q = 0; q < NQ; q++) {
      const int idx = (int)threadIdx.x + q * C::THR, r = (int)(((float)idx + 0.5f) * rk4), k = 4 * (idx - r * k4);
      if (idx < C::ROWS * k4) { X[k][r] = v[q].x; X[k + 1][r] = v[q].y; X[k + 2][r] = v[q].z; X[k + 3][r] = v[q].w; }
    }
    return;
  }
  for (int i = threadIdx.x; i < C::ROWS * Kp; i += C::THR) {
    const int r = i / Kp, k = i - r * Kp;
    float v = 0.f;
    if (mean) {
      if (k < in_dim && sr.live(r)) v = (x[(size_t)sr.grow(r) * ld + k] - mean[k]) / stdv[k];
    } else if (k < K && sr.live(r)) v = x[(size_t)sr.grow(r) * ld + k];
    X[k][r] = v;
  }
}

// The phases of the kernels below.  Stamps: forward 0 .. 11, backward from stamp c0.
// forward, hidden layers: x slab -> h1 -> h2; returns behind the barrier that leaves h2 in the slab.  bits1 / bits2 (HBM) or rb1 / rb2 (the
// thread's registers, with RB) take the ReLU mask words
template <class C, bool RB, int XK>
__device__ __forceinline__ void fwd_hidden(StripLds<C>& L, const MlpStripFwd& a, const SlabRows<C>& sr, unsigned (&rb1)[C::CT], unsigned (&rb2)[C::CT]) {
  static_assert(XK <= SH && XK % SBK == 0, "the input slab is the last XK rows of the activation slab");
  float (*X)[C::LD] = &L.S[SH - XK];
  WOp<C> w;
  SCLK(0);
  wload<C>(w, a.w1t, SH, a.Dp, 0);   // (the first weights of a layer are in flight while the slab is staged / the previous epilogue runs)
  stage_input<C, XK>(X, a.x, a.ldx, a.Dp, sr, a.in_mean, a.in_std, a.in_dim);
  __syncthreads();
  SCLK(1);
  f32x16 acc[C::RT][C::CT];
  zero_acc<C>(acc);
  slab_mma<C>(X, a.Dp, a.w1t, SH, w, acc);
  wload<C>(w, a.w2t, SH, SH, 0);
  SCLK(2);
  __syncthreads();   // every wave is done with the input slab
  SCLK(3);
  store_act<C, true, RB ? 1 : 0>(L, acc, a.b1, true, nullptr, a.h1, sr, a.bits1, nullptr, rb1);
  SCLK(4);
  __syncthreads();
  SCLK(5);
  zero_acc<C>(acc);
  slab_mma<C>(L.S, SH, a.w2t, SH, w, acc);
  SCLK(6);
  __syncthreads();
  SCLK(7);
  store_act<C, true, RB ? 1 : 0>(L, acc, a.b2, true, nullptr, a.h2, sr, a.bits2, nullptr, rb2);
  SCLK(8);
  __syncthreads();
  SCLK(9);
}

// read-out: y = h2 W3^T + b3, N = O <= 32: one column tile.  The K range is cut into SH / SKQ partial products of SKQ k each
// (the same cut for every workgroup shape, so every shape returns the same bits); a wave takes QW consecutive ones for all
// row tiles, and the partials are summed in ascending k order afterwards.  Returns behind the barrier that leaves the partials in the
// slab's memory as P [SH / SKQ][ROWS][32].
template <class C>
__device__ __forceinline__ float (*fwd_readout_partials(StripLds<C>& L, const MlpStripFwd& a))[C::ROWS][32] {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, kh = lane >> 5;
  constexpr int NQ = SH / SKQ, QW = NQ / C::NW;
  f32x16 p[QW][C::RT];
#pragma unroll
  for (int q = 0; q < QW; q++)
#pragma unroll
    for (int i = 0; i < C::RT; i++)
#pragma unroll
      for (int r = 0; r < 16; r++) p[q][i][r] = 0.f;
#pragma unroll
  for (int q = 0; q < QW; q++) {
#pragma unroll 8
    for (int kk = 0; kk < SKQ / 2; kk++) {
      const int k = (wave * QW + q) * SKQ + kk * 2 + kh;
      const float bv = a.w3t[(size_t)k * a.Op + min(l31, a.O - 1)], b = l31 < a.O ? bv : 0.f;
#pragma unroll
      for (int i = 0; i < C::RT; i++) p[q][i] = __builtin_amdgcn_mfma_f32_32x32x2f32(L.S[k][32 * i + l31], b, p[q][i], 0, 0, 0);
    }
  }
  SCLK(10);
  __syncthreads();   // all waves are done with the slab: it now holds the partial products
  SCLK(11);
  float (*P)[C::ROWS][32] = reinterpret_cast<float (*)[C::ROWS][32]>(&L.S[0][0]);     // [NQ][ROWS][32]: NQ * ROWS * 128 B <= the slab
#pragma unroll
  for (int q = 0; q < QW; q++)
#pragma unroll
    for (int i = 0; i < C::RT; i++)
#pragma unroll
      for (int r = 0; r < 16; r++) P[wave * QW + q][32 * i + (r & 3) + 8 * (r >> 2) + 4 * kh][l31] = p[q][i][r];
  __syncthreads();
  return P;
}

// Read-out of the WIDE instantiations (XK > SXK).  For rows wider than SXK columns the path these kernels take over is the per-layer GEMM
// forward, whose read-out is ONE fmaf chain over k = 0 .. SH - 1 from +0 with the bias behind it -- the order of policy_step_wide
// (lhw_humanoid_rollout.hip) and of mlp_policy_ref_kernel too -- not the sum of SH / SKQ partial chains.  A chain cannot be cut over k between
// waves: wave i < RT runs row tile i's, one accumulator through SH / 2 MFMAs, and the other waves wait at the barrier.  Returns like
// fwd_readout_partials, P[0] [ROWS][32] holding the chains (the caller adds the bias) and no further partial.
template <class C>
__device__ __forceinline__ float (*fwd_readout_chain(StripLds<C>& L, const MlpStripFwd& a))[C::ROWS][32] {
  static_assert(C::RT <= C::NW, "a wave per row tile");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, kh = lane >> 5;
  f32x16 p;
#pragma unroll
  for (int r = 0; r < 16; r++) p[r] = 0.f;
  if (wave < C::RT) {
#pragma unroll 8
    for (int kk = 0; kk < SH / 2; kk++) {
      const int k = kk * 2 + kh;
      const float bv = a.w3t[(size_t)k * a.Op + min(l31, a.O - 1)], b = l31 < a.O ? bv : 0.f;
      p = __builtin_amdgcn_mfma_f32_32x32x2f32(L.S[k][32 * wave + l31], b, p, 0, 0, 0);
    }
  }
  SCLK(10);
  __syncthreads();   // all waves are done with the slab
  SCLK(11);
  float (*P)[C::ROWS][32] = reinterpret_cast<float (*)[C::ROWS][32]>(&L.S[0][0]);
  if (wave < C::RT) {
#pragma unroll
    for (int r = 0; r < 16; r++) P[0][32 * wave + (r & 3) + 8 * (r >> 2) + 4 * kh][l31] = p[r];
  }
  __syncthreads();
  return P;
}
// how many partials the read-out of an instantiation with input-slab capacity XK leaves in P: SH / SKQ (fwd_readout_partials), or the one chain
template <int XK> struct ReadoutParts { static constexpr int N = XK > SXK ? 1 : SH / SKQ; };

// backward layers from the dy slab in X (complete, behind a barrier; `w` holds the first K step of W3): dh2 = (dy W3) * (h2 > 0) ->
// dh1 = (dh2 W2) * (h1 > 0).  The masks: the activations h1 / h2, or their bits from HBM (bits1 / bits2) or, with RB, registers (rb1 / rb2)
template <class C, bool RB>
__device__ __forceinline__ void bwd_layers(StripLds<C>& L, WOp<C>& w, const float* __restrict__ w2, const float* __restrict__ w3, const int O,
                                           const SlabRows<C>& sr, const float* __restrict__ h1, const float* __restrict__ h2, float* __restrict__ dh2,
                                           float* __restrict__ dh1, const unsigned* __restrict__ bits1, const unsigned* __restrict__ bits2,
                                           unsigned (&rb1)[C::CT], unsigned (&rb2)[C::CT], const int c0) {
  float (*X)[C::LD] = &L.S[SH - SXK];
  SCLK(c0);
  f32x16 acc[C::RT][C::CT];
  zero_acc<C>(acc);
  slab_mma<C>(X, O, w3, SH, w, acc);                                        // dy W3: B[k = o][n] = W3[o][n]
  wload<C>(w, w2, SH, SH, 0);
  SCLK(c0 + 1);
  __syncthreads();
  SCLK(c0 + 2);
  store_act<C, true, RB ? 2 : 0>(L, acc, nullptr, false, h2, dh2, sr, nullptr, bits2, rb2);
  SCLK(c0 + 3);
  __syncthreads();
  SCLK(c0 + 4);
  zero_acc<C>(acc);
  slab_mma<C>(L.S, SH, w2, SH, w, acc);                                     // dh2 W2: B[k = o][n = i] = W2[o][i]
  SCLK(c0 + 5);
  store_act<C, false, RB ? 2 : 0>(L, acc, nullptr, false, h1, dh1, sr, nullptr, bits1, rb1);
  SCLK(c0 + 6);
}

// XK: capacity of the input slab, SXK or SXW
template <class C, int XK>
__global__ void __launch_bounds__(C::THR, 2) mlp_fwd_strip_kernel(MlpStripFwd a) {
  __shared__ StripLds<C> L;
  LHW_LDS_POISON(L);
  const int tid = threadIdx.x;
  const int row0 = (int)blockIdx.x * C::ROWS;
  const SlabRows<C> sr = SlabRows<C>::consecutive(row0, a.R);
  unsigned rb1[C::CT], rb2[C::CT];   // (RB = 0: never touched; see store_act_t)
  fwd_hidden<C, false, XK>(L, a, sr, rb1, rb2);
  float (*P)[C::ROWS][32] = ReadoutParts<XK>::N == 1 ? fwd_readout_chain<C>(L, a) : fwd_readout_partials<C>(L, a);
  constexpr int NQ = ReadoutParts<XK>::N;
  for (int i = tid; i < C::ROWS * 32; i += C::THR) {
    const int row = i >> 5, col = i & 31;
    if (col < a.O && row0 + row < a.R) {
      float s = P[0][row][col];
#pragma unroll
      for (int q = 1; q < NQ; q++) s += P[q][row][col];
      s += a.b3[col];
      a.y[(size_t)(row0 + row) * a.Op + col] = s;
      if (a.act) {   // Gaussian head (rollout inference): the action component here, its log-density term through P[0] (this
        float term;  // thread's own, now spent, entry) to the row's first thread below
        a.act[(size_t)(row0 + row) * a.O + col] = lhw_policy_sample(s, a.stdv[col], a.seed, a.env_base + (unsigned)(row0 + row), a.counter, col, a.deterministic, &term);
        P[0][row][col] = term;
      }
    }
  }
  SCLK(12);
  if (a.act) {
    __syncthreads();
    for (int row = tid; row < C::ROWS; row += C::THR)
      if (row0 + row < a.R) {
        float lp = 0.f;
        for (int k = 0; k < a.O; k++) lp += P[0][row][k];     // (the order of sample_kernel's sum)
        a.logp[row0 + row] = lp;
      }
  }
}

template <class C>
__global__ void __launch_bounds__(C::THR, 2) mlp_bwd_strip_kernel(MlpStripBwd a) {
  __shared__ StripLds<C> L;
  LHW_LDS_POISON(L);
  const SlabRows<C> sr = SlabRows<C>::consecutive((int)blockIdx.x * C::ROWS, a.R);
  float (*X)[C::LD] = &L.S[SH - SXK];
  WOp<C> w;
  SCLK(0);
  wload<C>(w, a.w3, SH, a.O, 0);
  stage_input<C, SXK>(X, a.dy, a.Op, a.O, sr);
  __syncthreads();
  unsigned rb1[C::CT], rb2[C::CT];   // (RB = 0: never touched; see store_act_t)
  bwd_layers<C, false>(L, w, a.w2, a.w3, a.O, sr, a.h1, a.h2, a.dh2, a.dh1, a.bits1, a.bits2, rb1, rb2, 1);
}

// One network's forward layers, PPO head and backward layers on a slab that stays in its workgroup (MlpStripTrain).  Against the
// forward launch -> ppo_loss_kernel -> backward launch it drops: one slab tear-down and set-up (each reached in lock-step by the two
// workgroups of a CU), the loss launch and its dependency edges, and the HBM round trips of y, dy and the mask bits.  Every product and
// every row's arithmetic is the other path's: the same fwd_hidden / fwd_readout_partials / bwd_layers on the same per-row fmaf chains, the same
// ascending-k sum of the read-out partials, lhw_ppo_head.h's head -- bit-identical h1, h2, y, dy, dh2, dh1.
// (XK = SXW, the wide instantiation: the other path is the per-layer GEMMs around ppo_loss_kernel's head and the read-out is fwd_readout_chain's single
// chain; the dy slab stays in the LAST SXK rows of S, so the backward half is the narrow kernel's text.)
//   read-out sum: y = sum of the partials + b3 -> P[0] in place (each thread its own entries) and, if asked for, HBM
//   head: a thread per minibatch row reads its y (and its twin's) from P[0], writes dy k-major into the input-slab region X (disjoint from
//         P[0]), zero-padded as stage_input would, and the row's loss terms / dstd to HBM
//   dy slab -> HBM once (the weight-gradient kernels read it), then bwd_layers with the mask words still in registers
// Stamps: forward 0 .. 11, 12 read-out sum done, 13 head done (behind the barrier), backward 14 .. 20.
template <class C, int CRITIC, int XK>
__global__ void __launch_bounds__(C::THR, 2) mlp_train_strip_kernel(MlpStripTrain t) {
  static_assert(C::RT == 2, "a twin slab is two row tiles");
  __shared__ StripLds<C> L;
  LHW_LDS_POISON(L);
  const MlpStripFwd& a = t.f;
  const int tid = threadIdx.x;
  const int nrow = t.twin0 > 0 ? 32 : C::ROWS;   // minibatch rows per slab
  const SlabRows<C> sr = t.twin0 > 0 ? SlabRows<C>::twins((int)blockIdx.x * 32, a.R, t.twin0) : SlabRows<C>::consecutive((int)blockIdx.x * C::ROWS, a.R);
  unsigned rb1[C::CT], rb2[C::CT];
  fwd_hidden<C, true, XK>(L, a, sr, rb1, rb2);
  float (*P)[C::ROWS][32] = ReadoutParts<XK>::N == 1 ? fwd_readout_chain<C>(L, a) : fwd_readout_partials<C>(L, a);
  constexpr int NQ = ReadoutParts<XK>::N;
  for (int i = tid; i < C::ROWS * 32; i += C::THR) {
    const int row = i >> 5, col = i & 31;
    if (col < a.O) {
      float s = P[0][row][col];
#pragma unroll
      for (int q = 1; q < NQ; q++) s += P[q][row][col];
      s += a.b3[col];
      if (a.y && sr.live(row)) a.y[(size_t)sr.grow(row) * a.Op + col] = s;
      P[0][row][col] = s;
    }
  }
  SCLK(12);
  WOp<C> w;
  wload<C>(w, t.w3, SH, a.O, 0);
  __syncthreads();   // y is complete in P[0]; the other partials are spent
  float (*X)[C::LD] = &L.S[SH - SXK];   // (the dy slab: the last SXK rows whatever XK, disjoint from P[0])
  const int Kp = (a.O + SBK - 1) & ~(SBK - 1), Kz = max(Kp, a.Op);
  if (tid < nrow) {
    const int m = (int)blockIdx.x * nrow + tid;
    const bool twin = t.twin0 > 0;
    if (m < a.R) {
      if (CRITIC) {
        float dv;
        const float e2 = lhw_ppo_critic_row(t.head, m, P[0][tid][0], &dv);
        X[0][tid] = dv;
        for (int k = 1; k < Kz; k++) X[k][tid] = 0.f;
        t.stat_rows[(size_t)t.stat_ld + m] = e2;
      } else {
        float st[NSTAT];
        lhw_ppo_actor_row(t.head, m, &P[0][tid][0], twin ? &P[0][32 + tid][0] : nullptr, &X[0][tid], twin ? &X[0][32 + tid] : nullptr, C::LD, st);
        for (int k = a.Op; k < Kz; k++) { X[k][tid] = 0.f; if (twin) X[k][32 + tid] = 0.f; }
#pragma unroll
        for (int k = 0; k < NSTAT; k++)
          if (k != 1) t.stat_rows[(size_t)k * t.stat_ld + m] = st[k];
      }
    } else {
      for (int k = 0; k < Kz; k++) { X[k][tid] = 0.f; if (twin) X[k][32 + tid] = 0.f; }
    }
  }
  __syncthreads();
  SCLK(13);
  for (int i = tid; i < C::ROWS * a.Op; i += C::THR) {
    const int row = i / a.Op, k = i - row * a.Op;
    if (sr.live(row)) t.dy[(size_t)sr.grow(row) * a.Op + k] = X[k][row];
  }
  bwd_layers<C, true>(L, w, t.w2, t.w3, a.O, sr, nullptr, nullptr, t.dh2, t.dh1, nullptr, nullptr, rb1, rb2, 14);
}

// the head on outputs in HBM, a thread per minibatch row: the unfused twin of mlp_train_strip_kernel's head (lhw_debug_mlp_train_strip)
template <int CRITIC>
__global__ void __launch_bounds__(256) ppo_head_rows_kernel(LhwPpoHead h, const float* y, int Op, int twin0, float* dy, float* stat_rows, int stat_ld) {
  const int m = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (m >= h.B) return;
  if (CRITIC) {
    float dv;
    stat_rows[(size_t)stat_ld + m] = lhw_ppo_critic_row(h, m, y[(size_t)m * Op], &dv);
    dy[(size_t)m * Op] = dv;
    for (int k = 1; k < Op; k++) dy[(size_t)m * Op + k] = 0.f;
  } else {
    float st[NSTAT];
    lhw_ppo_actor_row(h, m, y + (size_t)m * Op, y + ((size_t)twin0 + m) * Op, dy + (size_t)m * Op, dy + ((size_t)twin0 + m) * Op, 1, st);
    for (int k = 0; k < NSTAT; k++)
      if (k != 1) stat_rows[(size_t)k * stat_ld + m] = st[k];
  }
}

// WT [cols][rows] <- W [rows][ld] for three matrices in one launch (the forward pass multiplies by W^T: its weight operand must
// have the output unit contiguous); 32 x 32 tiles through LDS, block b of matrix m handles tile b - first[m]
struct TransposeJob { const float* W; float* WT; int rows, cols, ld, ldt, first; };
struct TransposeJobs { TransposeJob j[3]; };
__global__ void __launch_bounds__(256) transpose3_kernel(TransposeJobs J) {
  __shared__ float T[32][33];
  LHW_LDS_POISON(T);
  const int b = (int)blockIdx.x, m = b >= J.j[2].first ? 2 : (b >= J.j[1].first ? 1 : 0);
  const TransposeJob q = J.j[m];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
  const int tc = (q.cols + 31) / 32, t = b - q.first, r0 = (t / tc) * 32, c0 = (t % tc) * 32;
  for (int y = ty; y < 32; y += 8) T[y][tx] = (r0 + y < q.rows && c0 + tx < q.cols) ? q.W[(size_t)(r0 + y) * q.ld + c0 + tx] : 0.f;
  __syncthreads();
  for (int y = ty; y < 32; y += 8)
    if (c0 + y < q.cols && r0 + tx < q.rows) q.WT[(size_t)(c0 + y) * q.ldt + r0 + tx] = T[tx][y];
}

size_t mlp_strip_wt_floats(int Dp, int Op) { return (size_t)Dp * SH + (size_t)SH * SH + (size_t)SH * Op; }

// transposed copies of the three weight matrices ([in][out]) for the forward strip kernel, into wt (mlp_strip_wt_floats floats)
void mlp_strip_prepare(const float* w1, const float* w2, const float* w3, int Dp, int O, int Op, float* wt, hipStream_t s) {
  float *w1t = wt, *w2t = wt + (size_t)Dp * SH, *w3t = w2t + (size_t)SH * SH;
  auto tiles = [](int rows, int cols) { return ((rows + 31) / 32) * ((cols + 31) / 32); };
  TransposeJobs J;
  J.j[0] = TransposeJob{w1, w1t, SH, Dp, Dp, SH, 0};
  J.j[1] = TransposeJob{w2, w2t, SH, SH, SH, SH, tiles(SH, Dp)};
  J.j[2] = TransposeJob{w3, w3t, O, SH, SH, Op, tiles(SH, Dp) + tiles(SH, SH)};
  hipLaunchKernelGGL(transpose3_kernel, dim3(J.j[2].first + tiles(O, SH)), dim3(256), 0, s, J);
}

void lhw_transpose3(const LhwTransposeJob (&jobs)[3], hipStream_t s) {
  TransposeJobs J;
  int first = 0;
  for (int m = 0; m < 3; m++) {
    J.j[m] = TransposeJob{jobs[m].W, jobs[m].WT, jobs[m].rows, jobs[m].cols, jobs[m].ld, jobs[m].ldt, first};
    first += ((jobs[m].rows + 31) / 32) * ((jobs[m].cols + 31) / 32);
  }
  if (first > 0) hipLaunchKernelGGL(transpose3_kernel, dim3(first), dim3(256), 0, s, J);
}

size_t mlp_strip_bits_words(size_t rows) { return (rows + StripBig::ROWS - 1) / StripBig::ROWS * StripBig::THR * StripBig::CT; }

// the narrow instantiations (input slab of SXK columns; read-out as partial sums) ...
bool mlp_strip_supported(int H, int Dp, int O, int Op) { return H == SH && Dp > 0 && Dp <= SXK && (Dp & 3) == 0 && O > 0 && O <= 32 && Op >= O; }
// ... and the wide ones (rows of an observation history: the input fills the slab; read-out as the GEMM path's single chain)
bool mlp_strip_wide_supported(int H, int Dp, int O, int Op) { return H == SH && Dp > SXK && Dp <= SXW && (Dp & 3) == 0 && O > 0 && O <= 32 && Op >= O; }

// Rows up to which the small shape is used: below it the slabs of the big shape would not even fill the CUs once, and the call
// is latency-bound (rollout inference); above it the big shape's operand reuse wins (the update's minibatches).
#define STRIP_SMALL_ROWS 16384
void mlp_strip_forward(const MlpStripFwd& a, hipStream_t s, int shape /* 0: by row count, 1: small, 2: big */) {
  if (a.R <= 0) return;
  const bool small = (shape == 1 || (shape == 0 && a.R <= STRIP_SMALL_ROWS)) && !a.bits1 && !a.bits2;   // (mask bits: the backward kernel's shape)
  const bool wide = a.Dp > SXK;                                                                         // (the instantiation by input width)
  const dim3 grid(small ? (a.R + StripSmall::ROWS - 1) / StripSmall::ROWS : (a.R + StripBig::ROWS - 1) / StripBig::ROWS), block(small ? StripSmall::THR : StripBig::THR);
  if (small && !wide) hipLaunchKernelGGL((mlp_fwd_strip_kernel<StripSmall, SXK>), grid, block, 0, s, a);
  else if (small) hipLaunchKernelGGL((mlp_fwd_strip_kernel<StripSmall, SXW>), grid, block, 0, s, a);
  else if (!wide) hipLaunchKernelGGL((mlp_fwd_strip_kernel<StripBig, SXK>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((mlp_fwd_strip_kernel<StripBig, SXW>), grid, block, 0, s, a);
}

void mlp_strip_backward(const MlpStripBwd& a, hipStream_t s) {
  if (a.R <= 0) return;
  hipLaunchKernelGGL((mlp_bwd_strip_kernel<StripBig>), dim3((a.R + StripBig::ROWS - 1) / StripBig::ROWS), dim3(StripBig::THR), 0, s, a);
}

// (the head keeps dy's slab in the input-slab region: Op <= SXK; the critic head is ppo_loss_kernel's: one value in rows of four)
bool mlp_train_strip_supported(int H, int Dp, int O, int Op, int critic) {
  return mlp_strip_supported(H, Dp, O, Op) && Op <= SXK && (!critic || (O == 1 && Op == 4));
}
bool mlp_train_strip_wide_supported(int H, int Dp, int O, int Op, int critic) {
  return mlp_strip_wide_supported(H, Dp, O, Op) && Op <= SXK && (!critic || (O == 1 && Op == 4));
}

void mlp_train_strip(const MlpStripTrain& t, hipStream_t s) {
  if (t.f.R <= 0) return;
  const int nrow = t.twin0 > 0 ? 32 : StripBig::ROWS;
  const dim3 grid((t.f.R + nrow - 1) / nrow), block(StripBig::THR);
  const bool wide = t.f.Dp > SXK;
  if (t.critic && !wide) hipLaunchKernelGGL((mlp_train_strip_kernel<StripBig, 1, SXK>), grid, block, 0, s, t);
  else if (t.critic) hipLaunchKernelGGL((mlp_train_strip_kernel<StripBig, 1, SXW>), grid, block, 0, s, t);
  else if (!wide) hipLaunchKernelGGL((mlp_train_strip_kernel<StripBig, 0, SXK>), grid, block, 0, s, t);
  else hipLaunchKernelGGL((mlp_train_strip_kernel<StripBig, 0, SXW>), grid, block, 0, s, t);
}

// C [M][ldc] = epilogue(A [M][lda] B): a thread per output, ONE fmaf chain over ascending k from +0 -- what gemm_f32_kernel's MFMA loop computes --
// then its epilogue: + bias[n], ReLU, zero where mask[m][n] <= 0.  B[k][n] = Bm[k * sk + n * sn].  The per-layer GEMM path in independent code
// (this file is built without lhw_gemm.hip on the SIMT emulator): the reference of the wide train strip (lhw_debug_mlp_train_strip, fused = 0).
__global__ void __launch_bounds__(256) mlp_ref_layer_kernel(int M, int N, int K, const float* __restrict__ A, int lda, const float* __restrict__ Bm, int sk, int sn,
                                                            float* __restrict__ C, int ldc, const float* __restrict__ bias, int relu,
                                                            const float* __restrict__ mask, int ldmask) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)M * N) return;
  const int m = (int)(i / N), n = (int)(i - (size_t)m * N);
  float v = 0.f;
  for (int k = 0; k < K; k++) v = fmaf(A[(size_t)m * lda + k], Bm[(size_t)k * sk + (size_t)n * sn], v);
  if (bias) v += bias[n];
  if (relu) v = fmaxf(v, 0.f);
  if (mask && !(mask[(size_t)m * ldmask + n] > 0.f)) v = 0.f;
  C[(size_t)m * ldc + n] = v;
}

// One network's forward + head + backward over a minibatch, outside an LhwPpo (tests, SIMT emulator).  fused = 1: mlp_train_strip_kernel.
// fused = 0: the forward strip launch(es), the head as a thread-per-row kernel on y in HBM, the backward strip launch(es) -- the reference
// the fused kernel must match bit for bit.
extern "C" int lhw_debug_mlp_train_strip(const LhwTrainStripArgs* q, int32_t fused, void* stream) {
  if (!q || !q->w1 || !q->b1 || !q->w2 || !q->b2 || !q->w3 || !q->b3 || !q->x || !q->h1 || !q->h2 || !q->y || !q->dy || !q->dh2 || !q->dh1 ||
      !q->stat_rows || !q->wt_scratch || (q->critic ? !q->ret : (!q->act || !q->old_logp || !q->adv || !q->stdv)))
    return lhw_fail(LHW_ERR_ARG, "null argument");
  const bool wide = mlp_train_strip_wide_supported(q->H, q->Dp, q->O, q->Op, q->critic);
  if ((!wide && !mlp_train_strip_supported(q->H, q->Dp, q->O, q->Op, q->critic)) || q->ldx < q->Dp || (q->ldx & 3))
    return lhw_fail(LHW_ERR_UNSUPPORTED, "train strip kernel: hidden width 256, padded input width <= %d (a multiple of 4), outputs <= 32 in rows of <= 64, critic 1 in 4", SXW);
  const int mir = !q->critic && q->twin0 > 0;
  if (q->B <= 0 || q->stat_ld < q->B || (mir && (q->twin0 < q->B || !q->act_src || !q->act_sign))) return lhw_fail(LHW_ERR_ARG, "bad row counts / mirror tables");
  hipStream_t s = (hipStream_t)stream;
  const int Dp = q->Dp, O = q->O, Op = q->Op, B = q->B;
  mlp_strip_prepare(q->w1, q->w2, q->w3, Dp, O, Op, q->wt_scratch, s);
  const float *w1t = q->wt_scratch, *w2t = w1t + (size_t)Dp * SH, *w3t = w2t + (size_t)SH * SH;
  const LhwPpoHead h{B, O, Op, q->act, q->old_logp, q->adv, q->ret, q->stdv, q->clip, q->mirror_coeff, mir, q->act_src, q->act_sign, q->dstd,
                     nullptr, nullptr, 0.f, 0.f, 1.f};
  if (fused) {
    MlpStripTrain t{MlpStripFwd{w1t, q->b1, w2t, q->b2, w3t, q->b3, q->x, q->ldx, Dp, O, Op, B, q->h1, q->h2, q->y}, q->w2, q->w3, q->dy, q->dh2, q->dh1,
                    mir ? q->twin0 : 0, q->critic, h, q->stat_rows, q->stat_ld};
    mlp_train_strip(t, s);
  } else if (wide) {
    // the path the wide train strip takes over: one GEMM per layer (mlp_forward / mlp_backward of lhw_ppo.hip without strips), here as plain chains
    auto layer = [&](int M, int N, int K, const float* A, int lda, const float* Bm, int sk, int sn, float* C, int ldc, const float* bias, int relu, const float* mask) {
      hipLaunchKernelGGL(mlp_ref_layer_kernel, dim3((unsigned)(((size_t)M * N + 255) / 256)), dim3(256), 0, s, M, N, K, A, lda, Bm, sk, sn, C, ldc, bias, relu, mask, SH);
    };
    for (int pass = 0; pass <= mir; pass++) {
      const size_t r0 = pass ? (size_t)q->twin0 : 0;
      layer(B, SH, Dp, q->x + r0 * q->ldx, q->ldx, q->w1, 1, Dp, q->h1 + r0 * SH, SH, q->b1, 1, nullptr);   // (weights in torch layout: B[k][n] = W[n][k])
      layer(B, SH, SH, q->h1 + r0 * SH, SH, q->w2, 1, SH, q->h2 + r0 * SH, SH, q->b2, 1, nullptr);
      layer(B, O, SH, q->h2 + r0 * SH, SH, q->w3, 1, SH, q->y + r0 * Op, Op, q->b3, 0, nullptr);
    }
    if (q->critic) hipLaunchKernelGGL(ppo_head_rows_kernel<1>, dim3((B + 255) / 256), dim3(256), 0, s, h, q->y, Op, 0, q->dy, q->stat_rows, q->stat_ld);
    else hipLaunchKernelGGL(ppo_head_rows_kernel<0>, dim3((B + 255) / 256), dim3(256), 0, s, h, q->y, Op, q->twin0, q->dy, q->stat_rows, q->stat_ld);
    for (int pass = 0; pass <= mir; pass++) {
      const size_t r0 = pass ? (size_t)q->twin0 : 0;
      layer(B, SH, O, q->dy + r0 * Op, Op, q->w3, SH, 1, q->dh2 + r0 * SH, SH, nullptr, 0, q->h2 + r0 * SH);   // dh2 = (dy W3) * (h2 > 0): B[k = o][n] = W3[o][n]
      layer(B, SH, SH, q->dh2 + r0 * SH, SH, q->w2, SH, 1, q->dh1 + r0 * SH, SH, nullptr, 0, q->h1 + r0 * SH);  // dh1 = (dh2 W2) * (h1 > 0)
    }
  } else {
    for (int pass = 0; pass <= mir; pass++) {
      const size_t r0 = pass ? (size_t)q->twin0 : 0;
      MlpStripFwd a{w1t, q->b1, w2t, q->b2, w3t, q->b3, q->x + r0 * q->ldx, q->ldx, Dp, O, Op, B, q->h1 + r0 * SH, q->h2 + r0 * SH, q->y + r0 * Op};
      mlp_strip_forward(a, s, 2);
    }
    if (q->critic) hipLaunchKernelGGL(ppo_head_rows_kernel<1>, dim3((B + 255) / 256), dim3(256), 0, s, h, q->y, Op, 0, q->dy, q->stat_rows, q->stat_ld);
    else hipLaunchKernelGGL(ppo_head_rows_kernel<0>, dim3((B + 255) / 256), dim3(256), 0, s, h, q->y, Op, q->twin0, q->dy, q->stat_rows, q->stat_ld);
    for (int pass = 0; pass <= mir; pass++) {
      const size_t r0 = pass ? (size_t)q->twin0 : 0;
      MlpStripBwd a{q->w2, q->w3, q->dy + r0 * Op, q->h1 + r0 * SH, q->h2 + r0 * SH, O, Op, B, q->dh2 + r0 * SH, q->dh1 + r0 * SH};
      mlp_strip_backward(a, s);
    }
  }
  return hipGetLastError() == hipSuccess ? LHW_OK : lhw_fail(LHW_ERR_HIP, "train strip launch failed");
}

extern "C" int lhw_debug_mlp_strip_forward_bits(int32_t H, int32_t Dp, int32_t O, int32_t Op, const float* w1, const float* b1, const float* w2,
                                                const float* b2, const float* w3, const float* b3, const float* x, int32_t ldx, int32_t R,
                                                float* h1, float* h2, float* y, float* wt_scratch, uint32_t* bits1, uint32_t* bits2, void* stream) {
  if (!wt_scratch || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !x || !h1 || !h2 || !y) return lhw_fail(LHW_ERR_ARG, "null argument");
  if ((!mlp_strip_supported(H, Dp, O, Op) && !mlp_strip_wide_supported(H, Dp, O, Op)) || ldx < Dp)
    return lhw_fail(LHW_ERR_UNSUPPORTED, "strip kernels: hidden width 256, padded input width <= %d (a multiple of 4), outputs <= 32", SXW);
  mlp_strip_prepare(w1, w2, w3, Dp, O, Op, wt_scratch, (hipStream_t)stream);
  MlpStripFwd a{wt_scratch, b1, wt_scratch + (size_t)Dp * SH, b2, wt_scratch + (size_t)Dp * SH + (size_t)SH * SH, b3, x, ldx, Dp, O, Op, R, h1, h2, y};
  a.bits1 = bits1; a.bits2 = bits2;
  const char* sh = getenv("LHW_DEBUG_STRIP_SHAPE");     // (tests: "small" / "big" force the workgroup shape; default by row count)
  mlp_strip_forward(a, (hipStream_t)stream, sh ? (sh[0] == 's' ? 1 : 2) : 0);
  return hipGetLastError() == hipSuccess ? LHW_OK : lhw_fail(LHW_ERR_HIP, "mlp_fwd_strip_kernel launch failed");
}
extern "C" int lhw_debug_mlp_strip_forward(int32_t H, int32_t Dp, int32_t O, int32_t Op, const float* w1, const float* b1, const float* w2,
                                           const float* b2, const float* w3, const float* b3, const float* x, int32_t ldx, int32_t R,
                                           float* h1, float* h2, float* y, float* wt_scratch, void* stream) {
  return lhw_debug_mlp_strip_forward_bits(H, Dp, O, Op, w1, b1, w2, b2, w3, b3, x, ldx, R, h1, h2, y, wt_scratch, nullptr, nullptr, stream);
}

extern "C" int lhw_debug_mlp_strip_backward_bits(int32_t H, int32_t O, int32_t Op, const float* w2, const float* w3, const float* dy, int32_t R,
                                                 const float* h1, const float* h2, float* dh2, float* dh1, const uint32_t* bits1, const uint32_t* bits2,
                                                 void* stream) {
  if (!w2 || !w3 || !dy || !dh2 || !dh1 || (!h1 && !bits1) || (!h2 && !bits2)) return lhw_fail(LHW_ERR_ARG, "null argument");
  if (!mlp_strip_supported(H, 4, O, Op)) return lhw_fail(LHW_ERR_UNSUPPORTED, "strip kernels: hidden width 256, outputs <= 32");
  MlpStripBwd a{w2, w3, dy, h1, h2, O, Op, R, dh2, dh1};
  a.bits1 = bits1; a.bits2 = bits2;
  mlp_strip_backward(a, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? LHW_OK : lhw_fail(LHW_ERR_HIP, "mlp_bwd_strip_kernel launch failed");
}
extern "C" int lhw_debug_mlp_strip_backward(int32_t H, int32_t O, int32_t Op, const float* w2, const float* w3, const float* dy, int32_t R,
                                            const float* h1, const float* h2, float* dh2, float* dh1, void* stream) {
  return lhw_debug_mlp_strip_backward_bits(H, O, Op, w2, w3, dy, R, h1, h2, dh2, dh1, nullptr, nullptr, stream);
}

// The feed-forward actor's policy step for rows WIDER than the strip kernels' SXK columns (an observation history, lhw_env_rollout_history) as a
// plain launch: a workgroup per row, a thread per hidden unit.  For such rows lhw_ppo_forward_at runs one GEMM per layer (mlp_forward, lhw_ppo.hip),
// so this is that path's order -- every layer ONE fmaf chain over ascending k from +0 (what gemm_f32_kernel's v_mfma_f32_32x32x2_f32 loop computes),
// then the bias, the read-out included -- and the order of policy_step_wide (lhw_humanoid_rollout.hip).  fp16_operands: as the in-wave step, every
// weight and activation rounded to fp16 before its product, float32 sums.
#if defined(__HIP_EMU__)
__device__ __forceinline__ float ref_r16(float x) { return emu_f16_round(x); }
#else
__device__ __forceinline__ float ref_r16(float x) { return (float)(_Float16)x; }
#endif
__global__ void __launch_bounds__(SH) mlp_policy_ref_kernel(LhwRolloutPolicy q, const float* __restrict__ obs, int R, unsigned env_base, unsigned counter,
                                                            float* __restrict__ y, float* __restrict__ act, float* __restrict__ logp) {
  __shared__ float xs[LHW_ROLLOUT_HISTORY_MAX_OBS_PAD], h1[SH], h2[SH], terms[32];   // (the whole row, at every width the launcher accepts: 6 KB with h1 / h2)
  LHW_LDS_POISON(xs);
  LHW_LDS_POISON(h1);
  LHW_LDS_POISON(h2);
  LHW_LDS_POISON(terms);
  const int row = (int)blockIdx.x, j = (int)threadIdx.x;
  const int D = q.obs_dim, Dp = q.obs_pad, O = q.act_dim, Op = q.act_pad;
  const bool half = q.fp16_operands != 0;
  for (int k = j; k < Dp; k += SH) {
    const float v = k < D ? (obs[(size_t)row * D + k] - q.obs_mean[k]) / q.obs_std[k] : 0.f;
    xs[k] = half ? ref_r16(v) : v;
  }
  __syncthreads();
  auto layer = [&](const float* wt, const float* bias, const float* x, int K) {
    float a = 0.f;
    for (int k = 0; k < K; k++) {
      const float w = wt[(size_t)k * SH + j];
      a = fmaf(half ? ref_r16(w) : w, x[k], a);
    }
    const float v = fmaxf(a + bias[j], 0.f);
    return half ? ref_r16(v) : v;
  };
  h1[j] = layer(q.w1t, q.b1, xs, Dp);
  __syncthreads();
  h2[j] = layer(q.w2t, q.b2, h1, SH);
  __syncthreads();
  if (j < O) {
    float s = 0.f;
    for (int k = 0; k < SH; k++) {
      const float w = q.w3t[(size_t)k * Op + j];
      s = fmaf(h2[k], half ? ref_r16(w) : w, s);
    }
    s += q.b3[j];
    y[(size_t)row * Op + j] = s;
    float term;
    act[(size_t)row * O + j] = lhw_policy_sample(s, q.stdv[j], q.seed, env_base + (unsigned)row, counter, j, q.deterministic, &term);
    terms[j] = term;
  }
  __syncthreads();
  if (j == 0) {
    float lp = 0.f;
    for (int k = 0; k < O; k++) lp += terms[k];     // (the order of sample_kernel's sum)
    logp[row] = lp;
  }
}

// the rollout's fused policy step (normalisation -> three layers -> Gaussian head) on R observation rows, from the actor view the
// resident rollout reads: the launch lhw_ppo_forward_at issues per control step, reachable without an LhwPpo (tests, SIMT emulator)
extern "C" int lhw_debug_policy_step(const LhwRolloutPolicy* q, const float* obs, int32_t R, uint32_t env_id_base, uint32_t counter, float* y,
                                     float* act, float* logp, void* stream) {
  if (!q || !obs || !y || !act || !logp || R <= 0) return lhw_fail(LHW_ERR_ARG, "bad argument");
  if (q->obs_pad > SXK) {      // an observation history: wider than the strip kernels' slab
    if (q->hidden != SH || q->obs_pad > LHW_ROLLOUT_HISTORY_MAX_OBS_PAD || (q->obs_pad & 3) || q->obs_pad < q->obs_dim || q->act_dim <= 0 || q->act_dim > 32 ||
        q->act_pad < q->act_dim)
      return lhw_fail(LHW_ERR_UNSUPPORTED, "policy step: hidden width 256, padded input width <= %d, outputs <= 32", LHW_ROLLOUT_HISTORY_MAX_OBS_PAD);
    hipLaunchKernelGGL(mlp_policy_ref_kernel, dim3(R), dim3(SH), 0, (hipStream_t)stream, *q, obs, R, env_id_base, counter, y, act, logp);
    return hipGetLastError() == hipSuccess ? LHW_OK : lhw_fail(LHW_ERR_HIP, "mlp_policy_ref_kernel launch failed");
  }
  if (!mlp_strip_supported(q->hidden, q->obs_pad, q->act_dim, q->act_pad)) return lhw_fail(LHW_ERR_UNSUPPORTED, "strip kernels: hidden width 256, padded input width <= 64, outputs <= 32");
  MlpStripFwd a{q->w1t, q->b1, q->w2t, q->b2, q->w3t, q->b3, obs, q->obs_dim, q->obs_pad, q->act_dim, q->act_pad, R, nullptr, nullptr, y};
  a.in_mean = q->obs_mean; a.in_std = q->obs_std; a.in_dim = q->obs_dim;
  a.stdv = q->stdv; a.act = act; a.logp = logp;
  a.seed = q->seed; a.env_base = env_id_base; a.counter = counter; a.deterministic = q->deterministic;
  const char* sh = getenv("LHW_DEBUG_STRIP_SHAPE");
  mlp_strip_forward(a, (hipStream_t)stream, sh ? (sh[0] == 's' ? 1 : 2) : 0);
  return hipGetLastError() == hipSuccess ? LHW_OK : lhw_fail(LHW_ERR_HIP, "mlp_fwd_strip_kernel launch failed");
}

// The LSTM actor's rollout step as a plain launch: a workgroup per row, a thread per hidden unit (all four gates of it), the chains of
// lstm_policy_step (lhw_humanoid_rollout.hip) and of lhw_rnn_forward's MFMA GEMMs -- one fmaf chain per gate pre-activation over ascending
// k of [x | h_prev] from +0 -- and the shared cell function.
#define LSH 256
#define LSXK 64
__global__ void __launch_bounds__(LSH) lstm_policy_ref_kernel(LhwRolloutLstmPolicy q, const float* __restrict__ obs, int R, const unsigned char* __restrict__ reset,
                                                              unsigned env_base, unsigned counter, float* __restrict__ y, float* __restrict__ act,
                                                              float* __restrict__ logp) {
  __shared__ float xs[LSXK], h1[LSH], h2[LSH], terms[32];
  LHW_LDS_POISON(xs);
  LHW_LDS_POISON(h1);
  LHW_LDS_POISON(h2);
  LHW_LDS_POISON(terms);
  const int row = (int)blockIdx.x, j = (int)threadIdx.x;
  const int D = q.obs_dim, Dp = q.obs_pad, O = q.act_dim, Op = q.act_pad;
  const bool rst = reset && reset[row];
  if (j < LSXK) xs[j] = j < D ? (obs[(size_t)row * D + j] - q.obs_mean[j]) / q.obs_std[j] : 0.f;
  h1[j] = rst ? 0.f : q.h1[(size_t)row * q.h1_ld + j];
  h2[j] = rst ? 0.f : q.h2[(size_t)row * q.h2_ld + j];
  __syncthreads();
  auto cell = [&](const float* wt, const float* xa, int Ka, const float* xb, const float* bi, const float* bh, float* c) {
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < Ka; k++)
      for (int n = 0; n < 4; n++) g[n] = fmaf(wt[(size_t)k * 4 * LSH + n * LSH + j], xa[k], g[n]);
    for (int k = 0; k < LSH; k++)
      for (int n = 0; n < 4; n++) g[n] = fmaf(wt[(size_t)(Ka + k) * 4 * LSH + n * LSH + j], xb[k], g[n]);
    const float b_ih[4] = {bi[j], bi[LSH + j], bi[2 * LSH + j], bi[3 * LSH + j]}, b_hh[4] = {bh[j], bh[LSH + j], bh[2 * LSH + j], bh[3 * LSH + j]};
    float gt[4], cn;
    const float h = lhw_lstm_cell(g[0], g[1], g[2], g[3], b_ih, b_hh, rst ? 0.f : c[(size_t)row * LSH + j], gt, &cn);
    c[(size_t)row * LSH + j] = cn;
    return h;
  };
  const float hn1 = cell(q.w1t, xs, Dp, h1, q.bi1, q.bh1, q.c1);
  __syncthreads();
  h1[j] = hn1;
  q.h1[(size_t)row * q.h1_ld + j] = hn1;
  __syncthreads();
  const float hn2 = cell(q.w2t, h1, LSH, h2, q.bi2, q.bh2, q.c2);
  __syncthreads();
  h2[j] = hn2;
  q.h2[(size_t)row * q.h2_ld + j] = hn2;
  __syncthreads();
  if (j < O) {
    float s = 0.f;
    for (int k = 0; k < LSH; k++) s = fmaf(h2[k], q.wot[(size_t)k * Op + j], s);
    s += q.bo[j];
    y[(size_t)row * Op + j] = s;
    float term;
    act[(size_t)row * O + j] = lhw_policy_sample(s, q.stdv[j], q.seed, env_base + (unsigned)row, counter, j, q.deterministic, &term);
    terms[j] = term;
  }
  __syncthreads();
  if (j == 0) {
    float lp = 0.f;
    for (int k = 0; k < O; k++) lp += terms[k];     // (the order of sample_kernel's sum)
    logp[row] = lp;
  }
}

extern "C" int lhw_debug_lstm_policy_step(const LhwRolloutLstmPolicy* q, const float* obs, int32_t R, const uint8_t* reset, uint32_t env_id_base,
                                          uint32_t counter, float* y, float* act, float* logp, void* stream) {
  if (!q || !obs || !y || !act || !logp || R <= 0) return lhw_fail(LHW_ERR_ARG, "bad argument");
  if (q->hidden != LSH || q->obs_pad > LSXK || (q->obs_pad & 3) || q->obs_pad < q->obs_dim || q->act_dim > 32 || q->act_pad < q->act_dim)
    return lhw_fail(LHW_ERR_UNSUPPORTED, "LSTM policy step: hidden width 256, padded input width <= 64, outputs <= 32");
  if (R > q->state_rows) return lhw_fail(LHW_ERR_ARG, "R = %d rows, the view's state holds %d", R, q->state_rows);
  hipLaunchKernelGGL(lstm_policy_ref_kernel, dim3(R), dim3(LSH), 0, (hipStream_t)stream, *q, obs, R, reset, env_id_base, counter, y, act, logp);
  return hipGetLastError() == hipSuccess ? LHW_OK : lhw_fail(LHW_ERR_HIP, "lstm_policy_ref_kernel launch failed");
}

// =========================================================================================== whole-sequence LSTM strip kernels
// The time loops of the recurrent update (lhw_rnn_grad, lhw_rnn.hip; reference rl/algos/ppo.py:512-533, the BPTT over whole trajectories of
// Gaussian_LSTM_Actor / LSTM_V) for one network as ONE launch per pass instead of four launches per time step.  The rows of a sequence
// minibatch are independent -- a row's h_t, c_t depend on its own x_t, h_{t-1}, c_{t-1} and the weights -- so a workgroup that owns a slab of
// 32 rows b of the [T][Bt] minibatch runs all T steps by itself: no grid synchronisation, no flag, no waiting on another workgroup.
//
// Workgroup = H / 32 waves (64 .. 512 threads); wave w owns the hidden units 32 w .. 32 w + 31 of both cells.  As in the MLP strips above the
// weights are the MFMA's A operand, read from global memory (L2) with the output unit contiguous, and the slab, k-major in LDS (S[k][row]),
// is its B operand, so lane l of an accumulator tile owns slab row l % 32 and the units 8 g + 4 (l / 32) + 0..3 of register quad g.
//   forward   per step and cell the wave multiplies FOUR tiles -- the gate columns j, H + j, 2H + j, 3H + j of its units -- over ascending k of
//             [x_t | h1_{t-1}] resp. [h1_t | h2_{t-1}]: every gate pre-activation is the fmaf chain from +0 that gemm_f32_kernel computes, all
//             four gates of a (row, unit) land in ONE lane, and lhw_lstm_cell runs on the accumulators.  c1 / c2 stay in registers for the whole
//             sequence, h1_t / h2_t reach the next product through the LDS slabs [Dp + H][32] and [2H][32]; x_{t+1} is staged while cell 1's
//             epilogue runs.  Three barriers per step.  Every buffer of SeqWs is written exactly as the launch-per-step loop writes it.
//   backward  t = T - 1 .. 0: lhw_lstm_cell_bwd for cell 2 on values from HBM, d [h1_t | h2_{t-1}] = dG2 W2 (two tiles per wave: its units of
//             d h1_t and of d h2_{t-1}), cell 1 on the first tile, d h1_{t-1} = dG1 W1[:, Dp:] (one tile).  The outputs of both products land in
//             the lanes that need them next, so the two d c carries and the two d h carries never leave registers; LDS holds only the product's
//             operand, the slab's d pre-activations [4H][32] (128 KB at H = 256), written by the cell phase as it stores them to g1 / g2.
//             Four barriers per step.
// Rows beyond Bt in the last slab load nothing and store nothing (their slab entries are zeros).
#define QH 256          // largest hidden width (8 waves)
#define QDP 128         // largest padded input width: (QDP + 3 QH) * 128 B + 16 KB of biases = 128 KB of LDS forward, 4 QH * 128 B = 128 KB backward, of 160 KB
#define QCH 4           // MFMAs (k pairs) per weight register buffer

struct SeqFwdLds { float S1[QDP + QH][32]; float S2[2 * QH][32]; float B[4][4 * QH]; };   // B: b_ih1, b_hh1, b_ih2, b_hh2
struct SeqBwdLds { float G[4 * QH][32]; };

// the wave's index as a value the compiler knows to be uniform: the weight addresses built from it are scalar bases plus one 32-bit lane offset
#ifdef __HIP_EMU__
#define SEQ_WAVE() ((int)(threadIdx.x >> 6))
#else
#define SEQ_WAVE() __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))
#endif

__device__ __forceinline__ void seq_zero(f32x16& acc) {
#pragma unroll
  for (int r = 0; r < 16; r++) acc[r] = 0.f;
}

// acc[q] += (S[0 .. K)[32 rows] ^T Bg[0 .. K)[n0[q] .. n0[q] + 32))^T for the wave's NT tiles: chains over ascending k, two k per MFMA.  K even.
// The weights of the next QCH k pairs are in flight while the current ones are multiplied (loads clamped to the last k pair, products guarded).
// n0 must be wave-uniform (SEQ_WAVE).
template <int NT>
__device__ __forceinline__ void seq_mma(const float (*S)[32], const int K, const float* __restrict__ Bg, const int ldb, const int (&n0)[NT], f32x16 (&acc)[NT]) {
  const int lane = threadIdx.x & 63, l31 = lane & 31, kh = lane >> 5;
  const unsigned voff = (unsigned)(kh * ldb + l31);
  float w0[QCH][NT], w1[QCH][NT];
  auto load = [&](float (&w)[QCH][NT], const int k0) {
#pragma unroll
    for (int kk = 0; kk < QCH; kk++) {
      const float* __restrict__ row = Bg + (size_t)min(k0 + 2 * kk, K - 2) * ldb;
#pragma unroll
      for (int q = 0; q < NT; q++) w[kk][q] = (row + n0[q])[voff];
    }
  };
  auto mul = [&](const float (&w)[QCH][NT], const int k0) {
#pragma unroll
    for (int kk = 0; kk < QCH; kk++)
      if (k0 + 2 * kk < K) {
        const float s = S[k0 + 2 * kk + kh][l31];
#pragma unroll
        for (int q = 0; q < NT; q++) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[kk][q], s, acc[q], 0, 0, 0);
      }
  };
  load(w0, 0);
  for (int k0 = 0; k0 < K; k0 += 4 * QCH) {
    load(w1, k0 + 2 * QCH);
    __builtin_amdgcn_sched_barrier(0);
    mul(w0, k0);
    __builtin_amdgcn_sched_barrier(0);
    load(w0, k0 + 4 * QCH);
    __builtin_amdgcn_sched_barrier(0);
    mul(w1, k0 + 2 * QCH);
    __builtin_amdgcn_sched_barrier(0);
  }
}

__device__ __forceinline__ void seq_ld4(float (&v)[4], const float* __restrict__ p) {
  const float4 t = *reinterpret_cast<const float4*>(p);
  v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
__device__ __forceinline__ void seq_st4(float* __restrict__ p, const float (&v)[4]) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }

// One cell's forward epilogue on the wave's four gate tiles: lhw_lstm_cell per (row, unit); activated gates -> G, c -> C, h -> dest_a (always)
// and dest_b (the next step's recurrent slot, zeroed where that step starts an episode; NULL at the last step), for live rows; h k-major into
// the slabs sa (NULL: not needed) and sb (with dest_b's zeroing).  row: this lane's row r of the step's [Bt][.] blocks.  bi / bh: the bias vectors
// in LDS (read from global memory they are loop-invariant loads, which the compiler hoists out of the time loop -- 256 values per lane: 79 spilled VGPRs)
// WS = false (lstm_seq_value_strip_kernel): nothing goes to HBM, only the slabs are written; keep: c stays as it is (an evaluation that does
// not advance the state).
template <bool WS = true>
__device__ __forceinline__ void seq_cell_fwd(const f32x16 (&acc)[4], float (&c)[16], const float* bi, const float* bh, const int H,
                                             const bool first, const bool rst, const bool rnext, const bool live, const size_t row,
                                             float* __restrict__ G, float* __restrict__ C, float* __restrict__ dest_a, const int lda,
                                             float* __restrict__ dest_b, const int ldb, float (*sa)[32], float (*sb)[32], const bool keep = false) {
  const int lane = threadIdx.x & 63, wave = SEQ_WAVE(), l31 = lane & 31, kh = lane >> 5;
#pragma unroll
  for (int g = 0; g < 4; g++) {
    const int j0 = 32 * wave + 8 * g + 4 * kh;
    float b_i[4][4], b_h[4][4], gt[4][4], hv[4], hz[4], cv[4];
#pragma unroll
    for (int q = 0; q < 4; q++) { seq_ld4(b_i[q], bi + q * H + j0); seq_ld4(b_h[q], bh + q * H + j0); }
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const int r = 4 * g + e;
      const float b_ih[4] = {b_i[0][e], b_i[1][e], b_i[2][e], b_i[3][e]}, b_hh[4] = {b_h[0][e], b_h[1][e], b_h[2][e], b_h[3][e]};
      float gq[4], cn;
      hv[e] = lhw_lstm_cell(acc[0][r], acc[1][r], acc[2][r], acc[3][r], b_ih, b_hh, (first || rst) ? 0.f : c[r], gq, &cn);
      if (!keep) c[r] = cn;
      cv[e] = cn;
      hz[e] = rnext ? 0.f : hv[e];
      gt[0][e] = gq[0]; gt[1][e] = gq[1]; gt[2][e] = gq[2]; gt[3][e] = gq[3];
      if (sa) sa[j0 + e][l31] = hv[e];
      if (sb) sb[j0 + e][l31] = hz[e];
      __builtin_amdgcn_sched_barrier(0);
    }
    if (WS && live) {
#pragma unroll
      for (int q = 0; q < 4; q++) seq_st4(G + row * 4 * H + q * H + j0, gt[q]);
      seq_st4(C + row * H + j0, cv);
      seq_st4(dest_a + row * lda + j0, hv);
      if (dest_b) seq_st4(dest_b + row * ldb + j0, hz);
    }
    __builtin_amdgcn_sched_barrier(0);   // one register quad at a time
  }
}

__global__ void __launch_bounds__(2 * QH) lstm_seq_fwd_strip_kernel(LstmSeqStrip a) {
  __shared__ SeqFwdLds L;
  LHW_LDS_POISON(L);
  const int tid = threadIdx.x, lane = tid & 63, wave = SEQ_WAVE(), l31 = lane & 31, nthr = (int)blockDim.x;
  const int H = a.H, Dp = a.Dp, K1 = Dp + H, Bt = a.Bt, T = a.T;
  const int b0 = (int)blockIdx.x * 32, b = b0 + l31;
  const bool live = b < Bt;
  // x_t of the slab's rows, k-major, zeros for the rows beyond Bt
  auto stage_x = [&](const int t) {
    for (int i = tid; i < 32 * Dp; i += nthr) {
      const int row = i / Dp, k = i - row * Dp;
      L.S1[k][row] = b0 + row < Bt ? a.xh1[((size_t)t * Bt + b0 + row) * K1 + k] : 0.f;
    }
  };
  // the recurrent slots of step 0 start from zero: in the slabs and in the workspaces (the backward pass and the weight-gradient GEMMs read those)
  for (int i = tid; i < 4 * H; i += nthr) { L.B[0][i] = a.bi1[i]; L.B[1][i] = a.bh1[i]; L.B[2][i] = a.bi2[i]; L.B[3][i] = a.bh2[i]; }
  for (int i = tid; i < 32 * H; i += nthr) {
    L.S1[Dp + (i >> 5)][i & 31] = 0.f;
    L.S2[H + (i >> 5)][i & 31] = 0.f;
    const int row = i / H, k = i - row * H;
    if (b0 + row < Bt) { a.xh1[(size_t)(b0 + row) * K1 + Dp + k] = 0.f; a.xh2[(size_t)(b0 + row) * 2 * H + H + k] = 0.f; }
  }
  stage_x(0);
  __syncthreads();
  float c1[16], c2[16];
#pragma unroll
  for (int r = 0; r < 16; r++) { c1[r] = 0.f; c2[r] = 0.f; }
  const int n0[4] = {32 * wave, H + 32 * wave, 2 * H + 32 * wave, 3 * H + 32 * wave};
  for (int t = 0; t < T; t++) {
    const size_t row = (size_t)t * Bt + b;
    const bool last = t + 1 == T;
    const bool rst = live && a.reset[row] != 0, rnext = !last && live && a.reset[row + Bt] != 0;
    f32x16 acc[4];
#pragma unroll
    for (int q = 0; q < 4; q++) seq_zero(acc[q]);
    seq_mma<4>(L.S1, K1, a.w1t, 4 * H, n0, acc);
    __syncthreads();   // every wave is done with [x_t | h1_{t-1}]
    seq_cell_fwd(acc, c1, L.B[0], L.B[1], H, t == 0, rst, rnext, live, row, a.g1, a.c1, a.xh2, 2 * H, last ? (float*)nullptr : a.xh1 + (size_t)Bt * K1 + Dp, K1,
                 L.S2, last ? (float (*)[32])nullptr : &L.S1[Dp]);
    if (!last) stage_x(t + 1);
    __syncthreads();   // h1_t is in both slabs
#pragma unroll
    for (int q = 0; q < 4; q++) seq_zero(acc[q]);
    seq_mma<4>(L.S2, 2 * H, a.w2t, 4 * H, n0, acc);
    __syncthreads();   // every wave is done with [h1_t | h2_{t-1}]
    seq_cell_fwd(acc, c2, L.B[2], L.B[3], H, t == 0, rst, rnext, live, row, a.g2, a.c2, a.h2, H, last ? (float*)nullptr : a.xh2 + (size_t)Bt * 2 * H + H, 2 * H,
                 (float (*)[32])nullptr, last ? (float (*)[32])nullptr : &L.S2[H]);
  }
}

// The critic of a stored recurrent rollout (lhw_rnn_values): the forward kernel's decomposition -- its slabs, seq_mma<4> and seq_cell_fwd -- on RAW
// observations, from the state lhw_rnn_forward keeps between calls and back into it, with the read-out (ONE output) in the kernel; nothing of
// size T N H reaches HBM.  Per step t the values are, bit for bit, those of
//   lhw_rnn_forward(obs[t], reset = t ? done[t-1] != 0 : reset0, commit = 1) -> val[t];  lhw_rnn_forward(term_obs[t], commit = 0) -> vterm[t]
// and, behind the last step, lhw_rnn_forward(obs[T], commit = 0) -> vfinal.
//   state     S1[Dp ..) and S2[H ..) hold h1_{t-1} / h2_{t-1} NOT yet zeroed for the episode starts of step t, and c1 / c2 (registers) likewise:
//             an evaluation that does not advance (vterm[t], vfinal) needs the state as step t left it.  The zeroing for step t + 1 is a pass
//             of its own behind those evaluations, run only where a live row of the slab has done[t] set (c: seq_cell_fwd's rst).
//   side      the evaluation that does not advance: cell 1 on [x' | h1_t] with c1 kept, h1' into S2[0 .. H) -- h1_t there is dead once the
//             main cell-2 product is through, its live copy is S1[Dp ..) -- cell 2 on [h1' | h2_t] with c2 kept, h2' into S2[0 .. H) again
//             (h1' is dead behind the product), read-out from there.  No LDS beyond the forward slabs.
//   vterm     the env writes a terminal observation that differs from the next observation only where the episode ended.  In a slab-step in
//             which no live row has done[t] set, V(term_obs[t]) from the state after step t IS the main evaluation of step t + 1 (same
//             input, no reset): vterm[t] = val[t + 1], resp. vfinal behind the last step, and the side evaluation is skipped.
//   read-out  gemm_f32_kernel's chain for N = 1: fmaf over ascending k of h2 from +0, then the bias; lane r < 32 of wave 0 owns row r.
// Rows beyond N in the last slab load nothing and store nothing.
struct SeqValLds { SeqFwdLds F; float nm[2][QDP]; float wo[QH]; };   // nm: obs_mean, obs_std (loop-invariant, like the biases)

__global__ void __launch_bounds__(2 * QH) lstm_seq_value_strip_kernel(LstmSeqValues a) {
  __shared__ SeqValLds L;
  LHW_LDS_POISON(L);
  const int tid = threadIdx.x, lane = tid & 63, wave = SEQ_WAVE(), l31 = lane & 31, kh = lane >> 5, nthr = (int)blockDim.x;
  const int H = a.H, D = a.D, Dp = a.Dp, K1 = Dp + H, N = a.N, T = a.T;
  const int b0 = (int)blockIdx.x * 32, b = b0 + l31;
  const bool live = b < N;
  // one time slice of raw observations [N][D], normalised (normalize_ld_kernel's expression), k-major; zeros in the padded columns and dead rows
  auto stage_x = [&](const float* __restrict__ x) {
    for (int i = tid; i < 32 * Dp; i += nthr) {
      const int row = i / Dp, k = i - row * Dp;
      L.F.S1[k][row] = (b0 + row < N && k < D) ? (x[(size_t)(b0 + row) * D + k] - L.nm[0][k]) / L.nm[1][k] : 0.f;
    }
  };
  // the value of this lane's row from h2 in S[0 .. H) (tid < 32)
  auto readout = [&](const float (*S)[32]) {
    float s = 0.f;
    for (int k = 0; k < H; k++) s = fmaf(S[k][l31], L.wo[k], s);
    return s + a.bo[0];
  };
  for (int i = tid; i < 4 * H; i += nthr) { L.F.B[0][i] = a.bi1[i]; L.F.B[1][i] = a.bh1[i]; L.F.B[2][i] = a.bi2[i]; L.F.B[3][i] = a.bh2[i]; }
  for (int i = tid; i < D; i += nthr) { L.nm[0][i] = a.obs_mean[i]; L.nm[1][i] = a.obs_std[i]; }
  for (int i = tid; i < H; i += nthr) L.wo[i] = a.wo[i];
  // the state the last call left, zero for the rows that start an episode now
  for (int i = tid; i < 32 * H; i += nthr) {
    const int row = i / H, k = i - row * H;
    const bool keep = b0 + row < N && !(a.reset0 && a.reset0[b0 + row]);
    L.F.S1[Dp + k][row] = keep ? a.h1[(size_t)(b0 + row) * a.h1_ld + k] : 0.f;
    L.F.S2[H + k][row] = keep ? a.h2[(size_t)(b0 + row) * a.h2_ld + k] : 0.f;
  }
  float c1[16], c2[16];
#pragma unroll
  for (int g = 0; g < 4; g++) {
    const int j0 = 32 * wave + 8 * g + 4 * kh;
    float u[4] = {0.f, 0.f, 0.f, 0.f}, v[4] = {0.f, 0.f, 0.f, 0.f};
    if (live) { seq_ld4(u, a.c1 + (size_t)b * H + j0); seq_ld4(v, a.c2 + (size_t)b * H + j0); }
#pragma unroll
    for (int e = 0; e < 4; e++) { c1[4 * g + e] = u[e]; c2[4 * g + e] = v[e]; }
  }
  __syncthreads();   // mean / std are in LDS
  stage_x(a.obs);
  __syncthreads();
  const int n0[4] = {32 * wave, H + 32 * wave, 2 * H + 32 * wave, 3 * H + 32 * wave};
  float (*const none)[32] = nullptr;
  bool fill_prev = false;   // vterm[t - 1] takes val[t]: step t - 1 skipped its side evaluation
  for (int t = 0; t < T; t++) {
    const bool last = t + 1 == T;
    const bool rst = live && (t ? a.done[(size_t)(t - 1) * N + b] != 0 : (a.reset0 && a.reset0[b] != 0));
    const bool any_done = __any(live && a.done[(size_t)t * N + b] != 0) != 0;   // the same in every wave: each holds all 32 rows
    const bool fin = last && a.vfinal;
    const bool side_t = a.vterm && (any_done || (last && !fin));
    const float* xnext = a.obs + (size_t)(t + 1) * N * D;   // obs[t + 1]: the next step's input, or vfinal's
    f32x16 acc[4];
#pragma unroll
    for (int q = 0; q < 4; q++) seq_zero(acc[q]);
    seq_mma<4>(L.F.S1, K1, a.w1t, 4 * H, n0, acc);
    __syncthreads();   // every wave is done with [x_t | h1_{t-1}]
    seq_cell_fwd<false>(acc, c1, L.F.B[0], L.F.B[1], H, false, rst, false, live, 0, nullptr, nullptr, nullptr, 0, nullptr, 0, L.F.S2, &L.F.S1[Dp]);
    if (side_t) stage_x(a.term_obs + (size_t)t * N * D);
    else if (!last || fin) stage_x(xnext);
    __syncthreads();   // h1_t is in both slabs
#pragma unroll
    for (int q = 0; q < 4; q++) seq_zero(acc[q]);
    seq_mma<4>(L.F.S2, 2 * H, a.w2t, 4 * H, n0, acc);
    __syncthreads();   // every wave is done with [h1_t | h2_{t-1}]
    seq_cell_fwd<false>(acc, c2, L.F.B[2], L.F.B[3], H, false, rst, false, live, 0, nullptr, nullptr, nullptr, 0, nullptr, 0, none, &L.F.S2[H]);
    __syncthreads();   // h2_t is complete
    if (tid < 32) {
      const float v = readout(&L.F.S2[H]);
      if (live) {
        a.val[(size_t)t * N + b] = v;
        if (fill_prev) a.vterm[(size_t)(t - 1) * N + b] = v;
      }
    }
    // the evaluations that do not advance the state: V(term_obs[t]), and behind the last step V(obs[T])
    const int nside = (side_t ? 1 : 0) + (fin ? 1 : 0);
    for (int e = 0; e < nside; e++) {
      const bool is_term = side_t && e == 0;
#pragma unroll
      for (int q = 0; q < 4; q++) seq_zero(acc[q]);
      seq_mma<4>(L.F.S1, K1, a.w1t, 4 * H, n0, acc);
      __syncthreads();   // every wave is done with [x' | h1_t]
      seq_cell_fwd<false>(acc, c1, L.F.B[0], L.F.B[1], H, false, false, false, live, 0, nullptr, nullptr, nullptr, 0, nullptr, 0, L.F.S2, none, true);
      if (is_term && (!last || fin)) stage_x(xnext);
      __syncthreads();   // h1' is in S2[0 .. H)
#pragma unroll
      for (int q = 0; q < 4; q++) seq_zero(acc[q]);
      seq_mma<4>(L.F.S2, 2 * H, a.w2t, 4 * H, n0, acc);
      __syncthreads();   // every wave is done with [h1' | h2_t]
      seq_cell_fwd<false>(acc, c2, L.F.B[2], L.F.B[3], H, false, false, false, live, 0, nullptr, nullptr, nullptr, 0, nullptr, 0, L.F.S2, none, true);
      __syncthreads();   // h2' is in S2[0 .. H)
      if (tid < 32) {
        const float v = readout(L.F.S2);
        if (live) {
          if (is_term) a.vterm[(size_t)t * N + b] = v;
          else {
            a.vfinal[b] = v;
            if (a.vterm && !side_t) a.vterm[(size_t)t * N + b] = v;
          }
        }
      }
    }
    fill_prev = a.vterm && !side_t;
    if (!last && any_done) {   // the rows whose episode ended start step t + 1 from zero
      __syncthreads();   // the read-outs are through with the slabs
      for (int i = tid; i < 32 * H; i += nthr) {
        const int k = i >> 5, row = i & 31;
        if (b0 + row < N && a.done[(size_t)t * N + b0 + row] != 0) { L.F.S1[Dp + k][row] = 0.f; L.F.S2[H + k][row] = 0.f; }
      }
      __syncthreads();
    }
  }
  // the state behind step T - 1, as lhw_rnn_forward(commit = 1) leaves it (no zeroing for done[T - 1]: that is the next call's reset0)
  for (int i = tid; i < 32 * H; i += nthr) {
    const int row = i / H, k = i - row * H;
    if (b0 + row < N) {
      a.h1[(size_t)(b0 + row) * a.h1_ld + k] = L.F.S1[Dp + k][row];
      a.h2[(size_t)(b0 + row) * a.h2_ld + k] = L.F.S2[H + k][row];
    }
  }
  if (live) {
#pragma unroll
    for (int g = 0; g < 4; g++) {
      const int j0 = 32 * wave + 8 * g + 4 * kh;
      const float u[4] = {c1[4 * g], c1[4 * g + 1], c1[4 * g + 2], c1[4 * g + 3]}, v[4] = {c2[4 * g], c2[4 * g + 1], c2[4 * g + 2], c2[4 * g + 3]};
      seq_st4(a.c1 + (size_t)b * H + j0, u);
      seq_st4(a.c2 + (size_t)b * H + j0, v);
    }
  }
}

// One cell's backward on the lane's (row, units): activated gates from G, c / c_prev from C, dh_a from DH [R][H] in HBM (cell 2) or, DH == NULL,
// from the accumulator tile dacc (cell 1), dh_b / the d c carry from registers; d pre-activation -> G (live rows) and k-major into the slab S
// (zeros for the rows beyond Bt)
__device__ __forceinline__ void seq_cell_bwd(const float* __restrict__ DH, const f32x16& dacc, const float (&dhb)[16], float (&dcar)[16], const int H, const bool first, const bool rst,
                                             const bool no_next, const bool live, const size_t row, const int Bt, float* __restrict__ G,
                                             const float* __restrict__ C, float (*S)[32]) {
  const int lane = threadIdx.x & 63, wave = SEQ_WAVE(), l31 = lane & 31, kh = lane >> 5;
#pragma unroll
  for (int g = 0; g < 4; g++) {
    const int j0 = 32 * wave + 8 * g + 4 * kh;
    float gt[4][4], cv[4], cp[4], d[4][4], dha[4];
#pragma unroll
    for (int e = 0; e < 4; e++) { cv[e] = 0.f; cp[e] = 0.f; gt[0][e] = 0.f; gt[1][e] = 0.f; gt[2][e] = 0.f; gt[3][e] = 0.f; dha[e] = DH ? 0.f : dacc[4 * g + e]; }
    if (live) {
      if (DH) seq_ld4(dha, DH + row * H + j0);
#pragma unroll
      for (int q = 0; q < 4; q++) seq_ld4(gt[q], G + row * 4 * H + q * H + j0);
      seq_ld4(cv, C + row * H + j0);
      if (!first) seq_ld4(cp, C + (row - Bt) * H + j0);
    }
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const int r = 4 * g + e;
      const float gq[4] = {gt[0][e], gt[1][e], gt[2][e], gt[3][e]};
      float dq[4];
      lhw_lstm_cell_bwd(gq, cv[e], cp[e], rst, dha[e], dhb[r], no_next, &dcar[r], dq);
#pragma unroll
      for (int q = 0; q < 4; q++) { d[q][e] = dq[q]; S[q * H + j0 + e][l31] = dq[q]; }
      __builtin_amdgcn_sched_barrier(0);
    }
    if (live) {
#pragma unroll
      for (int q = 0; q < 4; q++) seq_st4(G + row * 4 * H + q * H + j0, d[q]);
    }
    __builtin_amdgcn_sched_barrier(0);   // (as in seq_cell_fwd)
  }
}

__global__ void __launch_bounds__(2 * QH) lstm_seq_bwd_strip_kernel(LstmSeqStrip a) {
  __shared__ SeqBwdLds L;
  LHW_LDS_POISON(L);
  const int tid = threadIdx.x, lane = tid & 63, wave = SEQ_WAVE(), l31 = lane & 31;
  const int H = a.H, Dp = a.Dp, K1 = Dp + H, Bt = a.Bt, T = a.T;
  const int b = (int)blockIdx.x * 32 + l31;
  const bool live = b < Bt;
  float dc1[16], dc2[16], dh1c[16], dh2c[16];   // the carries: d c of both cells, d h1_t / d h2_t from step t + 1
#pragma unroll
  for (int r = 0; r < 16; r++) { dc1[r] = 0.f; dc2[r] = 0.f; dh1c[r] = 0.f; dh2c[r] = 0.f; }
  const int n2[2] = {32 * wave, H + 32 * wave}, n1[1] = {Dp + 32 * wave};
  for (int t = T - 1; t >= 0; t--) {
    const size_t row = (size_t)t * Bt + b;
    const bool last = t + 1 == T;
    const bool rst = live && a.reset[row] != 0, no_next = last || (live && a.reset[row + Bt] != 0);
    f32x16 acc2[2];
    seq_cell_bwd(a.dh2, acc2[0], dh2c, dc2, H, t == 0, rst, no_next, live, row, Bt, a.g2, a.c2, L.G);
    __syncthreads();   // dG2 of the slab is in LDS
    seq_zero(acc2[0]); seq_zero(acc2[1]);
    seq_mma<2>(L.G, 4 * H, a.w2, 2 * H, n2, acc2);       // d [h1_t | h2_{t-1}] = dG2 W2
#pragma unroll
    for (int r = 0; r < 16; r++) dh2c[r] = acc2[1][r];
    __syncthreads();   // every wave is done with dG2
    seq_cell_bwd(nullptr, acc2[0], dh1c, dc1, H, t == 0, rst, no_next, live, row, Bt, a.g1, a.c1, L.G);
    __syncthreads();   // dG1 of the slab is in LDS
    f32x16 acc1[1];
    seq_zero(acc1[0]);
    seq_mma<1>(L.G, 4 * H, a.w1, K1, n1, acc1);          // d h1_{t-1} = dG1 W1[:, Dp:]
#pragma unroll
    for (int r = 0; r < 16; r++) dh1c[r] = acc1[0][r];
    __syncthreads();   // every wave is done with dG1
  }
}

bool lstm_seq_strip_supported(int H, int Dp) {
  return H >= LHW_LSTM_SEQ_MIN_HIDDEN && H <= LHW_LSTM_SEQ_MAX_HIDDEN && H % 32 == 0 && Dp > 0 && Dp <= LHW_LSTM_SEQ_MAX_OBS_PAD && Dp % 4 == 0;
}
static_assert(LHW_LSTM_SEQ_MAX_HIDDEN == QH && LHW_LSTM_SEQ_MAX_OBS_PAD == QDP, "include/lhw.h states the kernels' bounds");

size_t lstm_seq_strip_wt_floats(int H, int Dp) { return (size_t)(Dp + H) * 4 * H + (size_t)2 * H * 4 * H; }

void lstm_seq_strip_prepare(const float* w1, const float* w2, int H, int Dp, float* wt, hipStream_t s) {
  const LhwTransposeJob jobs[3] = {{w1, wt, 4 * H, Dp + H, Dp + H, 4 * H}, {w2, wt + (size_t)(Dp + H) * 4 * H, 4 * H, 2 * H, 2 * H, 4 * H}, {nullptr, nullptr, 0, 0, 0, 0}};
  lhw_transpose3(jobs, s);
}

void lstm_seq_strip_forward(const LstmSeqStrip& a, hipStream_t s) {
  if (a.T <= 0 || a.Bt <= 0) return;
  hipLaunchKernelGGL(lstm_seq_fwd_strip_kernel, dim3((a.Bt + 31) / 32), dim3(2 * a.H), 0, s, a);
}
void lstm_seq_strip_backward(const LstmSeqStrip& a, hipStream_t s) {
  if (a.T <= 0 || a.Bt <= 0) return;
  hipLaunchKernelGGL(lstm_seq_bwd_strip_kernel, dim3((a.Bt + 31) / 32), dim3(2 * a.H), 0, s, a);
}

bool lstm_seq_values_supported(int H, int Dp) { return lstm_seq_strip_supported(H, Dp); }
void lstm_seq_strip_values(const LstmSeqValues& a, hipStream_t s) {
  if (a.T <= 0 || a.N <= 0) return;
  hipLaunchKernelGGL(lstm_seq_value_strip_kernel, dim3((a.N + 31) / 32), dim3(2 * a.H), 0, s, a);
}

// ---- the plain reference of lhw_debug_lstm_seq: the launch-per-step loops of lhw_rnn_grad (lhw_lstm_steps.h) with a thread per output in place of the MFMA GEMM
// C [M][N] (ld ldc) = A [M][K] (ld lda) B (+ bias [N] unless NULL), B[k][n] at B[k * sk + n * sn]: one fmaf chain over ascending k from +0 per output
__global__ void __launch_bounds__(256) seq_ref_gemm_kernel(int M, int N, int K, const float* __restrict__ A, int lda, const float* __restrict__ B, int sk, int sn,
                                                           float* __restrict__ C, int ldc, const float* __restrict__ bias) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)M * N) return;
  const int m = (int)(i / N), n = (int)(i - (size_t)m * N);
  float s = 0.f;
  for (int k = 0; k < K; k++) s = fmaf(A[(size_t)m * lda + k], B[(size_t)k * sk + (size_t)n * sn], s);
  C[(size_t)m * ldc + n] = bias ? s + bias[n] : s;   // (bias: gemm_f32_kernel's epilogue)
}

extern "C" int lhw_debug_lstm_seq(const LhwLstmSeqArgs* q, int32_t fused, void* stream) {
  if (!q || !q->w1 || !q->bi1 || !q->bh1 || !q->w2 || !q->bi2 || !q->bh2 || !q->reset || !q->xh1 || !q->xh2 || !q->g1 || !q->g2 || !q->c1 || !q->c2 || !q->h2 ||
      !q->scratch || ((q->passes & 2) && !q->dh2))
    return lhw_fail(LHW_ERR_ARG, "null argument");
  const int H = q->H, Dp = q->Dp, T = q->T, Bt = q->Bt, K1 = Dp + H;
  if (H <= 0 || Dp <= 0 || (Dp & 3) || T <= 0 || Bt <= 0 || !(q->passes & 3)) return lhw_fail(LHW_ERR_ARG, "bad shape (H=%d Dp=%d T=%d Bt=%d passes=%d)", H, Dp, T, Bt, q->passes);
  hipStream_t s = (hipStream_t)stream;
  if (fused) {
    if (!lstm_seq_strip_supported(H, Dp))
      return lhw_fail(LHW_ERR_UNSUPPORTED, "LSTM sequence strip kernels: hidden width a multiple of 32 in [%d, %d], padded input width <= %d", LHW_LSTM_SEQ_MIN_HIDDEN,
                      LHW_LSTM_SEQ_MAX_HIDDEN, LHW_LSTM_SEQ_MAX_OBS_PAD);
    const void* al[] = {q->bi1, q->bh1, q->bi2, q->bh2, q->xh1, q->xh2, q->g1, q->g2, q->c1, q->c2, q->h2, q->dh2};
    for (const void* p : al)
      if (reinterpret_cast<size_t>(p) & 15) return lhw_fail(LHW_ERR_ARG, "buffers must be 16-byte aligned");
    float* wt = q->scratch;
    LstmSeqStrip a{wt, wt + (size_t)K1 * 4 * H, q->w1, q->w2, q->bi1, q->bh1, q->bi2, q->bh2, q->xh1, q->xh2, q->g1, q->g2, q->c1, q->c2, q->h2, q->dh2, q->reset, T, Bt, H, Dp};
    if (q->passes & 1) {
      lstm_seq_strip_prepare(q->w1, q->w2, H, Dp, wt, s);
      lstm_seq_strip_forward(a, s);
    }
    if (q->passes & 2) lstm_seq_strip_backward(a, s);
    return hipGetLastError() == hipSuccess ? LHW_OK : lhw_fail(LHW_ERR_HIP, "LSTM sequence strip launch failed");
  }
  auto gemm = [&](int M, int N, int K, const float* A, int lda, const float* B, int ldb, bool b_kc, float* C, int ldc) {
    hipLaunchKernelGGL(seq_ref_gemm_kernel, dim3((unsigned)(((size_t)M * N + 255) / 256)), dim3(256), 0, s, M, N, K, A, lda, B, b_kc ? 1 : ldb, b_kc ? ldb : 1, C, ldc, (const float*)nullptr);
  };
  const LstmSeqStrip a{nullptr, nullptr, q->w1, q->w2, q->bi1, q->bh1, q->bi2, q->bh2, q->xh1, q->xh2, q->g1, q->g2, q->c1, q->c2, q->h2, q->dh2, q->reset, T, Bt, H, Dp};
  if (q->passes & 1) lstm_steps_forward(a, s, gemm);
  if (q->passes & 2) {
    float *dx2 = q->scratch, *dx1h = dx2 + (size_t)Bt * 2 * H, *dcar1 = dx1h + (size_t)Bt * H, *dcar2 = dcar1 + (size_t)Bt * H;
    lstm_steps_bptt(a, dx2, dx1h, dcar1, dcar2, s, gemm);
  }
  return hipGetLastError() == hipSuccess ? LHW_OK : lhw_fail(LHW_ERR_HIP, "LSTM sequence reference launch failed");
}

// The critic over a stored rollout outside an LhwRnn (tests, SIMT emulator).  fused = 1: lstm_seq_value_strip_kernel.  fused = 0: the calls it
// replaces -- lhw_rnn_forward's step (lstm_step_forward, lhw_lstm_steps.h) per time slice with a thread-per-output fmaf chain for the products.
extern "C" int lhw_debug_lstm_values(const LhwLstmValuesArgs* q, int32_t fused, void* stream) {
  if (!q || !q->w1 || !q->bi1 || !q->bh1 || !q->w2 || !q->bi2 || !q->bh2 || !q->wo || !q->bo || !q->obs_mean || !q->obs_std || !q->obs || !q->done || !q->xh1 ||
      !q->xh2 || !q->c1 || !q->c2 || !q->val || !q->scratch || (q->term_obs == nullptr) != (q->vterm == nullptr))
    return lhw_fail(LHW_ERR_ARG, "null argument");
  const int H = q->H, D = q->D, Dp = q->Dp, T = q->T, N = q->N, K1 = Dp + H;
  if (H <= 0 || D <= 0 || Dp < D || (Dp & 3) || T <= 0 || N <= 0) return lhw_fail(LHW_ERR_ARG, "bad shape (H=%d D=%d Dp=%d T=%d N=%d)", H, D, Dp, T, N);
  hipStream_t s = (hipStream_t)stream;
  if (fused) {
    if (!lstm_seq_values_supported(H, Dp))
      return lhw_fail(LHW_ERR_UNSUPPORTED, "LSTM value strip kernel: hidden width a multiple of 32 in [%d, %d], padded input width <= %d", LHW_LSTM_SEQ_MIN_HIDDEN,
                      LHW_LSTM_SEQ_MAX_HIDDEN, LHW_LSTM_SEQ_MAX_OBS_PAD);
    if ((reinterpret_cast<size_t>(q->c1) | reinterpret_cast<size_t>(q->c2)) & 15) return lhw_fail(LHW_ERR_ARG, "c1 / c2 must be 16-byte aligned");
    float* wt = q->scratch;
    lstm_seq_strip_prepare(q->w1, q->w2, H, Dp, wt, s);
    const LstmSeqValues a{wt, wt + (size_t)K1 * 4 * H, q->bi1, q->bh1, q->bi2, q->bh2, q->wo, q->bo, q->obs_mean, q->obs_std, q->obs, q->term_obs, q->done, q->reset0,
                          q->xh1 + Dp, K1, q->xh2 + H, 2 * H, q->c1, q->c2, q->val, q->vterm, q->vfinal, T, N, H, D, Dp};
    lstm_seq_strip_values(a, s);
    return hipGetLastError() == hipSuccess ? LHW_OK : lhw_fail(LHW_ERR_HIP, "LSTM value strip launch failed");
  }
  auto gemm = [&](int M, int Nn, int K, const float* A, int lda, const float* B, int ldb, bool b_kc, float* C, int ldc) {
    hipLaunchKernelGGL(seq_ref_gemm_kernel, dim3((unsigned)(((size_t)M * Nn + 255) / 256)), dim3(256), 0, s, M, Nn, K, A, lda, B, b_kc ? 1 : ldb, b_kc ? ldb : 1, C, ldc,
                       (const float*)nullptr);
  };
  float *g = q->scratch, *h2o = g + (size_t)N * 4 * H, *cs = h2o + (size_t)N * H;
  const LstmStepNet net{q->w1, q->bi1, q->bh1, q->w2, q->bi2, q->bh2, D, Dp, H};
  auto step = [&](const float* obs, const unsigned char* reset, bool commit, float* value) {
    lstm_step_forward(net, q->xh1, q->xh2, q->c1, q->c2, g, h2o, cs, obs, N, q->obs_mean, q->obs_std, reset, commit, s, gemm);
    hipLaunchKernelGGL(seq_ref_gemm_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, N, 1, H, (const float*)h2o, H, q->wo, 1, H, value, 1, q->bo);
  };
  for (int t = 0; t < T; t++) {
    step(q->obs + (size_t)t * N * D, t ? q->done + (size_t)(t - 1) * N : q->reset0, true, q->val + (size_t)t * N);
    if (q->vterm) step(q->term_obs + (size_t)t * N * D, nullptr, false, q->vterm + (size_t)t * N);
  }
  if (q->vfinal) step(q->obs + (size_t)T * N * D, nullptr, false, q->vfinal);
  return hipGetLastError() == hipSuccess ? LHW_OK : lhw_fail(LHW_ERR_HIP, "LSTM value reference launch failed");
}
