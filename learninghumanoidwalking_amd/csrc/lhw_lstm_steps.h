// The launch-per-step path of the recurrent update: the two cell kernels and the forward / BPTT time loops over them, written once for
// lhw_rnn_grad (lhw_rnn.hip, LHW_RNN_SEQ_FUSED=0 and shapes the strip kernels do not take; GEMM = the MFMA launch_gemm) and for the plain
// reference of lhw_debug_lstm_seq (lhw_mlp_strip.hip, which the SIMT emulator builds; GEMM = a thread per output).  The kernels are static:
// each of the two translation units carries its own copy of the one definition.
// Likewise the rollout step of one network (lstm_step_forward): lhw_rnn_forward's body, and the per-step reference of lhw_debug_lstm_values.
#pragma once
#include <hip/hip_runtime.h>

#include "lhw_internal.h"
#include "lhw_lstm_cell.h"

// gates G [B][4H] (pre-activation, biases not yet added) -> activated in place; c, h of this step (lhw_lstm_cell.h: the arithmetic of one unit).
// h goes to dest_a (always) and dest_b (zeroed for rows whose NEXT step starts an episode: the recurrent slot).
static __global__ void __launch_bounds__(256) lstm_cell_fwd_kernel(int B, int H, float* __restrict__ G, const float* __restrict__ bi,
                                                                   const float* __restrict__ bh, const float* __restrict__ c_prev,
                                                                   const unsigned char* __restrict__ reset_t, float* __restrict__ c_out,
                                                                   float* __restrict__ dest_a, int lda, float* __restrict__ dest_b, int ldb,
                                                                   const unsigned char* __restrict__ reset_next) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)B * H) return;
  const int b = (int)(i / H), j = (int)(i - (size_t)b * H);
  float* g = G + (size_t)b * 4 * H;
  const float cp = (c_prev && !(reset_t && reset_t[b])) ? c_prev[(size_t)b * H + j] : 0.f;
  const float b_ih[4] = {bi[j], bi[H + j], bi[2 * H + j], bi[3 * H + j]}, b_hh[4] = {bh[j], bh[H + j], bh[2 * H + j], bh[3 * H + j]};
  float gt[4], c;
  const float h = lhw_lstm_cell(g[j], g[H + j], g[2 * H + j], g[3 * H + j], b_ih, b_hh, cp, gt, &c);
  g[j] = gt[0]; g[H + j] = gt[1]; g[2 * H + j] = gt[2]; g[3 * H + j] = gt[3];
  c_out[(size_t)b * H + j] = c;
  dest_a[(size_t)b * lda + j] = h;
  if (dest_b) dest_b[(size_t)b * ldb + j] = (reset_next && reset_next[b]) ? 0.f : h;
}

// backward of one cell step: G holds the activated gates and receives d loss / d pre-activation; dcar carries d loss / d c
// to the previous step (zero across an episode start)
static __global__ void __launch_bounds__(256) lstm_cell_bwd_kernel(int B, int H, float* __restrict__ G, const float* __restrict__ c,
                                                                   const float* __restrict__ c_prev, const unsigned char* __restrict__ reset_t,
                                                                   const float* __restrict__ dh_a, int lda, const float* __restrict__ dh_b, int ldb,
                                                                   const unsigned char* __restrict__ reset_next, float* __restrict__ dcar) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)B * H) return;
  const int b = (int)(i / H), j = (int)(i - (size_t)b * H);
  float* g = G + (size_t)b * 4 * H;
  const float gt[4] = {g[j], g[H + j], g[2 * H + j], g[3 * H + j]};
  const bool rst = reset_t && reset_t[b];
  const float cp = (c_prev && !rst) ? c_prev[(size_t)b * H + j] : 0.f;
  const bool no_next = !dh_b || (reset_next && reset_next[b]);
  const float dhb = no_next ? 0.f : dh_b[(size_t)b * ldb + j];
  float dc = dcar[(size_t)b * H + j], d[4];
  lhw_lstm_cell_bwd(gt, c[(size_t)b * H + j], cp, rst, dh_a[(size_t)b * lda + j], dhb, no_next, &dc, d);
  dcar[(size_t)b * H + j] = dc;
  g[j] = d[0]; g[H + j] = d[1]; g[2 * H + j] = d[2]; g[3 * H + j] = d[3];
}

// p[b][0 .. H) = 0 for B rows of stride ld: the recurrent slots of step 0
static __global__ void __launch_bounds__(256) lstm_zero_slot_kernel(int B, int H, float* __restrict__ p, int ld) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < (size_t)B * H) p[(i / H) * ld + i % H] = 0.f;
}

// gemm(M, N, K, A, lda, B, ldb, b_kc, C, ldc): C [M][N] = A [M][K] op(B); b_kc: B is stored [N][K] (ld ldb), else [K][N].
// Forward time loop: four launches per step.  a.w1 / a.w2 are theta's own [4H][Dp + H] and [4H][2H]; a.w1t / a.w2t are not read.
template <class Gemm>
static void lstm_steps_forward(const LstmSeqStrip& a, hipStream_t s, Gemm gemm) {
  const int T = a.T, Bt = a.Bt, H = a.H, K1 = a.Dp + H;
  const int nb = (int)(((size_t)Bt * H + 255) / 256);
  // the recurrent slots of step 0 start from zero
  hipLaunchKernelGGL(lstm_zero_slot_kernel, dim3(nb), dim3(256), 0, s, Bt, H, a.xh1 + a.Dp, K1);
  hipLaunchKernelGGL(lstm_zero_slot_kernel, dim3(nb), dim3(256), 0, s, Bt, H, a.xh2 + H, 2 * H);
  for (int t = 0; t < T; t++) {
    const size_t r0 = (size_t)t * Bt;
    const bool last = t + 1 == T;
    const unsigned char* rnext = last ? nullptr : a.reset + r0 + Bt;
    gemm(Bt, 4 * H, K1, a.xh1 + r0 * K1, K1, a.w1, K1, true, a.g1 + r0 * 4 * H, 4 * H);
    hipLaunchKernelGGL(lstm_cell_fwd_kernel, dim3(nb), dim3(256), 0, s, Bt, H, a.g1 + r0 * 4 * H, a.bi1, a.bh1,
                       t ? a.c1 + (r0 - Bt) * H : (const float*)nullptr, a.reset + r0, a.c1 + r0 * H, a.xh2 + r0 * 2 * H, 2 * H,
                       last ? (float*)nullptr : a.xh1 + (r0 + Bt) * K1 + a.Dp, K1, rnext);
    gemm(Bt, 4 * H, 2 * H, a.xh2 + r0 * 2 * H, 2 * H, a.w2, 2 * H, true, a.g2 + r0 * 4 * H, 4 * H);
    hipLaunchKernelGGL(lstm_cell_fwd_kernel, dim3(nb), dim3(256), 0, s, Bt, H, a.g2 + r0 * 4 * H, a.bi2, a.bh2,
                       t ? a.c2 + (r0 - Bt) * H : (const float*)nullptr, a.reset + r0, a.c2 + r0 * H, a.h2 + r0 * H, H,
                       last ? (float*)nullptr : a.xh2 + (r0 + Bt) * 2 * H + H, 2 * H, rnext);
  }
}

// BPTT time loop given a.dh2: d loss / d pre-activation of every step into a.g1 / a.g2.  Per-step scratch: dx2 [Bt][2H], dx1h / dcar1 / dcar2 [Bt][H]
template <class Gemm>
static void lstm_steps_bptt(const LstmSeqStrip& a, float* dx2, float* dx1h, float* dcar1, float* dcar2, hipStream_t s, Gemm gemm) {
  const int T = a.T, Bt = a.Bt, H = a.H, K1 = a.Dp + H;
  const int nb = (int)(((size_t)Bt * H + 255) / 256);
  (void)hipMemsetAsync(dcar1, 0, sizeof(float) * Bt * H, s);
  (void)hipMemsetAsync(dcar2, 0, sizeof(float) * Bt * H, s);
  for (int t = T - 1; t >= 0; t--) {
    const size_t r0 = (size_t)t * Bt;
    const bool last = t + 1 == T;
    const unsigned char* rnext = last ? nullptr : a.reset + r0 + Bt;
    hipLaunchKernelGGL(lstm_cell_bwd_kernel, dim3(nb), dim3(256), 0, s, Bt, H, a.g2 + r0 * 4 * H, a.c2 + r0 * H,
                       t ? a.c2 + (r0 - Bt) * H : (const float*)nullptr, a.reset + r0, a.dh2 + r0 * H, H,
                       last ? (const float*)nullptr : dx2 + H, 2 * H, rnext, dcar2);
    gemm(Bt, 2 * H, 4 * H, a.g2 + r0 * 4 * H, 4 * H, a.w2, 2 * H, false, dx2, 2 * H);        // d [h1_t | h2_{t-1}] = dG2 W2
    hipLaunchKernelGGL(lstm_cell_bwd_kernel, dim3(nb), dim3(256), 0, s, Bt, H, a.g1 + r0 * 4 * H, a.c1 + r0 * H,
                       t ? a.c1 + (r0 - Bt) * H : (const float*)nullptr, a.reset + r0, dx2, 2 * H,
                       last ? (const float*)nullptr : dx1h, H, rnext, dcar1);
    gemm(Bt, H, 4 * H, a.g1 + r0 * 4 * H, 4 * H, a.w1 + a.Dp, K1, false, dx1h, H);           // d h1_{t-1} = dG1 W1[:, Dp:]
  }
}

// (obs - mean) / std written into the x part of a concatenated input buffer (row stride ld)
static __global__ void normalize_ld_kernel(const float* __restrict__ obs, int D, int Dp, size_t R, const float* __restrict__ mean,
                                           const float* __restrict__ stdv, float* __restrict__ out, int ld) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= R * (size_t)Dp) return;
  size_t r = i / Dp;
  int j = (int)(i - r * Dp);
  out[r * ld + j] = j < D ? (obs[r * D + j] - mean[j]) / stdv[j] : 0.f;
}
// zero the hidden / cell state of rows starting an episode
static __global__ void rnn_reset_kernel(int N, int H, const unsigned char* __restrict__ reset, float* __restrict__ h1, int ld1,
                                        float* __restrict__ h2, int ld2, float* __restrict__ c1, float* __restrict__ c2) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)N * H) return;
  const int b = (int)(i / H), j = (int)(i - (size_t)b * H);
  if (reset[b]) { h1[(size_t)b * ld1 + j] = 0.f; h2[(size_t)b * ld2 + j] = 0.f; c1[i] = 0.f; c2[i] = 0.f; }
}

// One network's rollout step on N rows, up to the top hidden state h2_out [N][H] (the read-out is the caller's).  The state between steps
// lives in the recurrent columns of the concatenated step inputs xh1 [N][Dp + H] = [x | h1], xh2 [N][2H] = [h1 | h2] and in c1 / c2 [N][H].
// reset ([N], may be NULL): rows that start an episode with this observation.  commit: the state advances; else it is only read (the new
// cell states go to cs [N][H]).  g: [N][4H] scratch.
struct LstmStepNet {
  const float *w1, *bi1, *bh1, *w2, *bi2, *bh2;   // theta's own [4H][Dp + H], [4H][2H], biases [4H]
  int D, Dp, H;
};
template <class Gemm>
static void lstm_step_forward(const LstmStepNet& n, float* xh1, float* xh2, float* c1, float* c2, float* g, float* h2_out, float* cs, const float* obs, int N,
                              const float* obs_mean, const float* obs_std, const unsigned char* reset, bool commit, hipStream_t s, Gemm gemm) {
  const int H = n.H, Dp = n.Dp, K1 = Dp + H;
  const int nb = (int)(((size_t)N * H + 255) / 256);
  if (reset && commit) hipLaunchKernelGGL(rnn_reset_kernel, dim3(nb), dim3(256), 0, s, N, H, reset, xh1 + Dp, K1, xh2 + H, 2 * H, c1, c2);
  const size_t nn = (size_t)N * Dp;
  hipLaunchKernelGGL(normalize_ld_kernel, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, s, obs, n.D, Dp, (size_t)N, obs_mean, obs_std, xh1, K1);
  gemm(N, 4 * H, K1, xh1, K1, n.w1, K1, true, g, 4 * H);
  hipLaunchKernelGGL(lstm_cell_fwd_kernel, dim3(nb), dim3(256), 0, s, N, H, g, n.bi1, n.bh1, (const float*)c1, (const unsigned char*)nullptr, commit ? c1 : cs,
                     xh2, 2 * H, commit ? xh1 + Dp : (float*)nullptr, K1, (const unsigned char*)nullptr);
  gemm(N, 4 * H, 2 * H, xh2, 2 * H, n.w2, 2 * H, true, g, 4 * H);
  hipLaunchKernelGGL(lstm_cell_fwd_kernel, dim3(nb), dim3(256), 0, s, N, H, g, n.bi2, n.bh2, (const float*)c2, (const unsigned char*)nullptr, commit ? c2 : cs,
                     h2_out, H, commit ? xh2 + H : (float*)nullptr, 2 * H, (const unsigned char*)nullptr);
}
