// On-device recurrent (LSTM) PPO: the learner handle LhwRnn, its rollout step and its BPTT update.
// Gaussian_LSTM_Actor / LSTM_V (reference rl/policies/actor.py:191-286, critic.py:52-112): two stacked LSTMCells and a
// linear read-out per network; rollout = one cell step per control step with the hidden state reset at episode starts
// (rl/workers/rollout_worker.py:134-137,174-177); update = back-propagation through time over whole trajectories
// (rl/algos/ppo.py:512-533).  Where the reference pads a list of trajectories to a common length and masks the losses,
// the device keeps the rollout's time-major layout: a minibatch is a set of env columns over all T steps, the hidden and
// cell state are zeroed wherever an episode starts inside a column, and every (t, column) sample is valid -- the same
// per-trajectory computation and the same loss mean, without padding.
//
// Per cell the input and recurrent weights are stored side by side, W = [W_ih | W_hh] ([4H][K], gate order i f g o as
// in torch), so one MFMA GEMM over the concatenated input [x_t | h_{t-1}] gives the gate pre-activations; the two bias
// vectors stay separate parameters (they receive the same gradient).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <memory>

#include "lhw_gemm.h"
#include "lhw_learner.h"
#include "lhw_lstm_steps.h"

struct LstmLayout {
  int D, Dp, H, O, Op, K1;
  size_t w1, bi1, bh1, w2, bi2, bh2, wo, bo, total;
};
static LstmLayout lstm_layout(int D, int H, int O) {
  LstmLayout L;
  L.D = D; L.Dp = pad4(D); L.H = H; L.O = O; L.Op = pad4(O); L.K1 = L.Dp + H;
  size_t o = 0;
  L.w1 = o; o += (size_t)4 * H * L.K1;
  L.bi1 = o; o += 4 * H;
  L.bh1 = o; o += 4 * H;
  L.w2 = o; o += (size_t)4 * H * 2 * H;
  L.bi2 = o; o += 4 * H;
  L.bh2 = o; o += 4 * H;
  L.wo = o; o += (size_t)L.Op * H;
  L.bo = o; o += L.Op;
  L.total = o;
  return L;
}

struct SeqWs {  // activations of one network over a [T][Bt] minibatch (rows r = t * Bt + b)
  float *xh1 = nullptr, *xh2 = nullptr;  // [R][K1] = [x_t | h1_{t-1}], [R][2H] = [h1_t | h2_{t-1}]
  float *g1 = nullptr, *g2 = nullptr;    // [R][4H] activated gates (overwritten by d loss / d pre-activation in the backward pass)
  float *c1 = nullptr, *c2 = nullptr;    // [R][H] cell states
  float *h2 = nullptr, *y = nullptr;     // [R][H] top hidden state, [R][Op] read-out
  float *dy = nullptr, *dh2 = nullptr;   // [R][Op], [R][H]
  float *dx2 = nullptr, *dx1h = nullptr, *dcar1 = nullptr, *dcar2 = nullptr;  // per-step scratch [Bt][2H], [Bt][H], [Bt][H] x2
  int Bt = 0;
};

struct LhwRnn : LearnerCore {
  int T, Bmax, Nroll;
  LstmLayout la, lc;
  // rollout: per network the concatenated step inputs hold the hidden state between calls, cells in rc
  float *rxh1[2] = {nullptr, nullptr}, *rxh2[2] = {nullptr, nullptr}, *rc1[2] = {nullptr, nullptr}, *rc2[2] = {nullptr, nullptr};
  float *rg = nullptr, *rh2 = nullptr, *ry = nullptr, *rcs = nullptr;  // step scratch: gates [N][4H], top hidden [N][H], read-out [N][Op], cells [N][H]
  SeqWs wa, wc;
  unsigned char* reset = nullptr;  // [T][Bmax]
  float *mb_act = nullptr, *mb_logp = nullptr, *mb_adv = nullptr, *mb_ret = nullptr, *dstd = nullptr;
  float *part = nullptr;
  float *wt_roll = nullptr;        // the actor's [in][out] weight copies for the resident rollout (lhw_rnn_rollout_policy), allocated by its first call
  // whole-sequence strip kernels (lhw_mlp_strip.hip) in place of the two time loops of lhw_rnn_grad: LHW_RNN_SEQ_FUSED / lhw_rnn_debug_set_seq_fused
  int seq_fused = 1;
  int last_grad_fused = 0;         // which path the last lhw_rnn_grad took (lhw_rnn_debug_last_grad_fused)
  float* wt_seq[2] = {nullptr, nullptr};   // [in][out] copies of W1cat, W2cat for the forward strip kernel (actor, critic), made once per lhw_rnn_grad; NULL: shape not covered
  hipStream_t side = nullptr;      // the critic's time loops run beside the actor's, as in lhw_ppo_grad
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  ~LhwRnn() {
    (void)hipSetDevice(device);
    if (side) { (void)hipStreamSynchronize(side); (void)hipStreamDestroy(side); }
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    if (ev_join) (void)hipEventDestroy(ev_join);
  }
};

// sequence minibatch gather: columns idx[0..B) of the time-major rollout [T][N] -> rows (t, b) of the workspaces
__global__ void seq_gather_kernel(const int* __restrict__ idx, int T, int N, int B, int Bt, int Dp, int K1, int A,
                                  const float* __restrict__ xn, const float* __restrict__ xm, const float* __restrict__ act,
                                  const float* __restrict__ logp, const float* __restrict__ adv, const float* __restrict__ ret,
                                  const unsigned char* __restrict__ done, float* __restrict__ xa, float* __restrict__ xc,
                                  float* __restrict__ mact, float* __restrict__ mlogp, float* __restrict__ madv,
                                  float* __restrict__ mret, unsigned char* __restrict__ reset_a, unsigned char* __restrict__ reset_c) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)T * B * Dp) return;
  const size_t m = i / Dp;
  const int j = (int)(i - m * Dp), t = (int)(m / B), b = (int)(m - (size_t)t * B);
  const size_t src = (size_t)t * N + idx[b];
  const float v = xn[src * Dp + j];
  xa[((size_t)t * Bt + b) * K1 + j] = v;
  if (xm) xa[((size_t)t * Bt + B + b) * K1 + j] = xm[src * Dp + j];
  xc[m * K1 + j] = v;
  if (j < A) mact[m * A + j] = act[src * A + j];
  if (j == 0) {
    mlogp[m] = logp[src]; madv[m] = adv[src]; mret[m] = ret[src];
    const unsigned char r = (t == 0 || done[(size_t)(t - 1) * N + idx[b]]) ? 1 : 0;   // an episode starts at step t of this column
    reset_a[(size_t)t * Bt + b] = r;
    if (xm) reset_a[(size_t)t * Bt + B + b] = r;
    reset_c[m] = r;
  }
}

static LstmSeqStrip seq_strip_args(const LstmLayout& L, const float* th, const SeqWs& w, int T, const unsigned char* reset, const float* wt) {
  return LstmSeqStrip{wt, wt ? wt + (size_t)L.K1 * 4 * L.H : nullptr, th + L.w1, th + L.w2, th + L.bi1, th + L.bh1, th + L.bi2, th + L.bh2,
                      w.xh1, w.xh2, w.g1, w.g2, w.c1, w.c2, w.h2, w.dh2, reset, T, w.Bt, L.H, L.Dp};
}
// C [M][N] = A [M][K] op(B), no epilogue: the GEMM of the launch-per-step loops (lhw_lstm_steps.h) and of the rollout step
static auto steps_gemm(hipStream_t s) {
  return [s](int M, int N, int K, const float* A, int lda, const float* B, int ldb, bool b_kc, float* C, int ldc) {
    GemmArgs g{};
    g.A = A; g.lda = lda; g.B = B; g.ldb = ldb; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K;
    if (b_kc) launch_gemm<true, true>(g, s);
    else launch_gemm<true, false>(g, s);
  };
}

// wt != NULL: the time loop as one launch (lstm_seq_fwd_strip_kernel; wt = the [in][out] weight copies), else four launches per step
static void lstm_seq_forward(const LstmLayout& L, const float* th, SeqWs& w, int T, const unsigned char* reset, hipStream_t s, const float* wt) {
  const LstmSeqStrip a = seq_strip_args(L, th, w, T, reset, wt);
  if (wt) lstm_seq_strip_forward(a, s);
  else lstm_steps_forward(a, s, steps_gemm(s));
  GemmArgs g{};
  g.A = w.h2; g.lda = L.H; g.B = th + L.wo; g.ldb = L.H; g.C = w.y; g.ldc = L.Op; g.M = T * w.Bt; g.N = L.O; g.K = L.H; g.bias = th + L.bo;
  launch_gemm<true, true>(g, s);
}

// BPTT given w.dy: d loss / d pre-activation of every step into w.g1 / w.g2 (wt != NULL: the time loop as one launch, lstm_seq_bwd_strip_kernel)
static void lstm_seq_bptt(const LstmLayout& L, const float* th, SeqWs& w, int T, const unsigned char* reset, hipStream_t s, const float* wt) {
  GemmArgs g{};
  g.A = w.dy; g.lda = L.Op; g.B = th + L.wo; g.ldb = L.H; g.C = w.dh2; g.ldc = L.H; g.M = T * w.Bt; g.N = L.H; g.K = L.O;
  launch_gemm<true, false>(g, s);
  const LstmSeqStrip a = seq_strip_args(L, th, w, T, reset, wt);
  if (wt) lstm_seq_strip_backward(a, s);
  else lstm_steps_bptt(a, w.dx2, w.dx1h, w.dcar1, w.dcar2, s, steps_gemm(s));
}

// accumulates the parameter gradients of this network into grad (same layout as theta): contractions over all R = T * Bt rows at once
static void lstm_seq_wgrad(const LstmLayout& L, float* grad, SeqWs& w, int T, float* part, int k_chunk, hipStream_t s) {
  const int Bt = w.Bt, H = L.H, K1 = L.K1, R = T * Bt;
  GemmArgs g{};
  g.A = w.g2; g.lda = 4 * H; g.B = w.xh2; g.ldb = 2 * H; g.C = grad + L.w2; g.ldc = 2 * H; g.M = 4 * H; g.N = 2 * H; g.K = R; g.part = part; g.k_chunk = k_chunk;
  launch_gemm<false, false>(g, s);
  colsum_det(w.g2, R, 4 * H, 4 * H, grad + L.bi2, part, s);
  colsum_det(w.g2, R, 4 * H, 4 * H, grad + L.bh2, part, s);
  g = GemmArgs{};
  g.A = w.g1; g.lda = 4 * H; g.B = w.xh1; g.ldb = K1; g.C = grad + L.w1; g.ldc = K1; g.M = 4 * H; g.N = K1; g.K = R; g.part = part; g.k_chunk = k_chunk;
  launch_gemm<false, false>(g, s);
  colsum_det(w.g1, R, 4 * H, 4 * H, grad + L.bi1, part, s);
  colsum_det(w.g1, R, 4 * H, 4 * H, grad + L.bh1, part, s);
  g = GemmArgs{};
  g.A = w.dy; g.lda = L.Op; g.B = w.h2; g.ldb = H; g.C = grad + L.wo; g.ldc = H; g.M = L.O; g.N = H; g.K = R; g.part = part; g.k_chunk = k_chunk;
  launch_gemm<false, false>(g, s);
  colsum_det(w.dy, R, L.Op, L.O, grad + L.bo, part, s);
}

extern "C" int lhw_rnn_destroy(LhwRnn* p) {
  delete p;
  return LHW_OK;
}

// seq_len / seq_cols: capacity of a BPTT minibatch (time steps x env columns); rollout_rows: envs stepped per call
extern "C" int lhw_rnn_create(const LhwPpoConfig* c, int32_t seq_len, int32_t seq_cols, int32_t rollout_rows, LhwRnn** out) {
  if (const int rc = learner_check(c, (void**)out, seq_len > 0 && seq_cols > 0 && rollout_rows > 0)) return rc;
  std::unique_ptr<LhwRnn> p(new LhwRnn());
  p->T = seq_len; p->Bmax = seq_cols; p->Nroll = rollout_rows;
  p->la = lstm_layout(c->obs_dim, c->hidden, c->act_dim);
  p->lc = lstm_layout(c->obs_dim, c->hidden, 1);
  learner_init(*p, c, p->la.total, p->lc.total);
  auto alloc = [&](auto** ptr, size_t n) { p->mem.get(ptr, n); };   // (zero-filled; one check of p->mem at the end)
  const size_t H = p->H, K1 = p->la.K1, Op = p->la.Op, N = p->Nroll;
  for (int n = 0; n < 2; n++) { alloc(&p->rxh1[n], N * K1); alloc(&p->rxh2[n], N * 2 * H); alloc(&p->rc1[n], N * H); alloc(&p->rc2[n], N * H); }
  alloc(&p->rg, N * 4 * H); alloc(&p->rh2, N * H); alloc(&p->ry, N * Op); alloc(&p->rcs, N * H);
  auto alloc_ws = [&](SeqWs& w, const LstmLayout& L, int Bt) {
    const size_t R = (size_t)p->T * Bt;
    w.Bt = Bt;
    alloc(&w.xh1, R * L.K1); alloc(&w.xh2, R * 2 * H); alloc(&w.g1, R * 4 * H); alloc(&w.g2, R * 4 * H); alloc(&w.c1, R * H); alloc(&w.c2, R * H);
    alloc(&w.h2, R * H); alloc(&w.y, R * L.Op); alloc(&w.dy, R * L.Op); alloc(&w.dh2, R * H);
    alloc(&w.dx2, (size_t)Bt * 2 * H); alloc(&w.dx1h, (size_t)Bt * H); alloc(&w.dcar1, (size_t)Bt * H); alloc(&w.dcar2, (size_t)Bt * H);
  };
  alloc_ws(p->wa, p->la, p->use_mirror ? 2 * p->Bmax : p->Bmax);
  alloc_ws(p->wc, p->lc, p->Bmax);
  const size_t Rm = (size_t)p->T * p->Bmax;
  alloc(&p->reset, 3 * Rm);   // actor rows (up to 2 Bmax per step) then critic rows
  alloc(&p->mb_act, Rm * p->A); alloc(&p->mb_logp, Rm); alloc(&p->mb_adv, Rm); alloc(&p->mb_ret, Rm); alloc(&p->dstd, Rm * Op);
  alloc(&p->stats, 16); alloc(&p->stats_part, ((Rm + 255) / 256) * NSTAT); alloc(&p->norm_part, 2 * SUMSQ_BLOCKS);
  const size_t max_slices = (2 * Rm + 2047) / 2048;
  alloc(&p->part, std::max<size_t>(max_slices * 4 * H * std::max<size_t>(K1, 2 * H), (size_t)COLSUM_CHUNKS * 4 * H));
  p->seq_fused = !(getenv("LHW_RNN_SEQ_FUSED") && atoi(getenv("LHW_RNN_SEQ_FUSED")) == 0);
  if (lstm_seq_strip_supported(p->H, p->la.Dp)) {
    for (int n = 0; n < 2; n++) alloc(&p->wt_seq[n], lstm_seq_strip_wt_floats(p->H, p->la.Dp));
    if (hipStreamCreateWithFlags(&p->side, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&p->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&p->ev_join, hipEventDisableTiming) != hipSuccess)
      return lhw_fail(LHW_ERR_HIP, "recurrent PPO: side stream / event creation failed");
  }
  if (p->mem.failed() || !learner_mirror(*p, c))
    return lhw_fail(LHW_ERR_HIP, "recurrent PPO workspace allocation failed (T=%d cols=%d) or bad mirror table", seq_len, seq_cols);
  *out = p.release();
  return LHW_OK;
}

extern "C" int lhw_rnn_debug_set_seq_fused(LhwRnn* p, int32_t on) {
  if (!p) return lhw_fail(LHW_ERR_ARG, "null argument");
  p->seq_fused = on ? 1 : 0;
  return LHW_OK;
}
extern "C" int lhw_rnn_debug_last_grad_fused(const LhwRnn* p) { return p ? p->last_grad_fused : LHW_ERR_ARG; }

extern "C" int64_t lhw_rnn_param_count(const LhwRnn* p) { return p ? (int64_t)p->n_params : LHW_ERR_ARG; }

// offsets in the flat parameter vector: out[0..7] actor W1 (cat) b_ih1 b_hh1 W2 (cat) b_ih2 b_hh2 Wout bout; out[8] stds;
// out[9..16] critic likewise; out[17] padded obs width Dp; out[18] padded actor read-out width Op
extern "C" int lhw_rnn_layout(const LhwRnn* p, int64_t* out19) {
  if (!p || !out19) return lhw_fail(LHW_ERR_ARG, "null argument");
  const LstmLayout* Ls[2] = {&p->la, &p->lc};
  const size_t off[2] = {p->off_actor, p->off_critic};
  for (int n = 0; n < 2; n++) {
    const LstmLayout& L = *Ls[n];
    const size_t v[8] = {L.w1, L.bi1, L.bh1, L.w2, L.bi2, L.bh2, L.wo, L.bo};
    for (int k = 0; k < 8; k++) out19[n * 9 + k] = (int64_t)(off[n] + v[k]);
  }
  out19[8] = (int64_t)p->off_std;
  out19[17] = p->la.Dp; out19[18] = p->la.Op;
  return LHW_OK;
}

// One rollout step for N rows.  reset (device, [N], may be NULL): rows that start an episode with this observation.
// commit != 0 advances the stored hidden / cell state (the reference's policy(state) / critic(state) calls in
// RolloutWorker.sample); commit == 0 evaluates without touching it (value of a terminal / final observation).
extern "C" int lhw_rnn_forward(LhwRnn* p, const float* theta, const float* obs, int64_t N, const float* obs_mean, const float* obs_std,
                               const uint8_t* reset, uint64_t seed, uint32_t env_id_base, uint32_t counter, int deterministic,
                               int commit, float* mu, float* act, float* logp, float* value, void* stream) {
  if (!p || !theta || !obs || N <= 0 || N > p->Nroll) return lhw_fail(LHW_ERR_ARG, "bad argument (N=%lld, capacity %d)", (long long)N, p ? p->Nroll : 0);
  if (act && !logp) return lhw_fail(LHW_ERR_ARG, "logp required with act");
  HIPCHK(hipSetDevice(p->device));
  hipStream_t s = (hipStream_t)stream;
  const int H = p->H, Dp = p->la.Dp;
  const bool want[2] = {act != nullptr || mu != nullptr, value != nullptr};
  const auto gemm = steps_gemm(s);
  for (int n = 0; n < 2; n++) {
    if (!want[n]) continue;
    const LstmLayout& L = n ? p->lc : p->la;
    const float* th = theta + (n ? p->off_critic : p->off_actor);
    const LstmStepNet net{th + L.w1, th + L.bi1, th + L.bh1, th + L.w2, th + L.bi2, th + L.bh2, p->D, Dp, H};
    lstm_step_forward(net, p->rxh1[n], p->rxh2[n], p->rc1[n], p->rc2[n], p->rg, p->rh2, p->rcs, obs, (int)N, obs_mean, obs_std, reset, commit != 0, s, gemm);
    GemmArgs g{};
    g.A = p->rh2; g.lda = H; g.B = th + L.wo; g.ldb = H; g.C = p->ry; g.ldc = L.Op; g.M = (int)N; g.N = L.O; g.K = H; g.bias = th + L.bo;
    launch_gemm<true, true>(g, s);
    if (n == 0) {
      if (mu) HIPCHK(hipMemcpy2DAsync(mu, sizeof(float) * p->A, p->ry, sizeof(float) * L.Op, sizeof(float) * p->A, N, hipMemcpyDeviceToDevice, s));
      if (act)
        hipLaunchKernelGGL(sample_kernel, dim3((N + 7) / 8), dim3(256), 0, s, p->ry, L.Op, p->A, (int)N, theta + p->off_std, seed, env_id_base,
                           counter, deterministic, act, logp);
    } else {
      HIPCHK(hipMemcpy2DAsync(value, sizeof(float), p->ry, sizeof(float) * L.Op, sizeof(float), N, hipMemcpyDeviceToDevice, s));
    }
  }
  HIPCHK(hipGetLastError());
  return LHW_OK;
}

// The critic over a stored rollout as one launch (lstm_seq_value_strip_kernel, lhw_mlp_strip.hip) in place of 2T + 1 calls of lhw_rnn_forward: same
// values, same state left in rxh1[1] / rxh2[1] / rc1[1] / rc2[1].  The [in][out] weight copies go to the scratch lhw_rnn_grad's critic strip uses
// (wt_seq[1]; every user fills it before reading it, in stream order).
extern "C" int lhw_rnn_values(LhwRnn* p, const float* theta, const float* obs, const float* term_obs, const uint8_t* done, const uint8_t* reset0, int32_t T,
                              int32_t N, const float* obs_mean, const float* obs_std, float* val, float* vterm, float* vfinal, void* stream) {
  if (!p || !theta || !obs || !done || !obs_mean || !obs_std || !val || (term_obs == nullptr) != (vterm == nullptr)) return lhw_fail(LHW_ERR_ARG, "null argument");
  if (T <= 0 || N <= 0 || N > p->Nroll) return lhw_fail(LHW_ERR_ARG, "bad argument (T=%d, N=%d, capacity %d)", T, N, p->Nroll);
  const LstmLayout& L = p->lc;
  if (!lstm_seq_values_supported(L.H, L.Dp) || !p->wt_seq[1])
    return lhw_fail(LHW_ERR_UNSUPPORTED, "lhw_rnn_values: hidden width a multiple of 32 in [%d, %d] (this critic: %d), padded observation width <= %d",
                    LHW_LSTM_SEQ_MIN_HIDDEN, LHW_LSTM_SEQ_MAX_HIDDEN, L.H, LHW_LSTM_SEQ_MAX_OBS_PAD);
  HIPCHK(hipSetDevice(p->device));
  hipStream_t s = (hipStream_t)stream;
  const float* th = theta + p->off_critic;
  float* wt = p->wt_seq[1];
  lstm_seq_strip_prepare(th + L.w1, th + L.w2, L.H, L.Dp, wt, s);
  const LstmSeqValues a{wt, wt + (size_t)L.K1 * 4 * L.H, th + L.bi1, th + L.bh1, th + L.bi2, th + L.bh2, th + L.wo, th + L.bo, obs_mean, obs_std, obs, term_obs, done, reset0,
                        p->rxh1[1] + L.Dp, L.K1, p->rxh2[1] + L.H, 2 * L.H, p->rc1[1], p->rc2[1], val, vterm, vfinal, T, N, L.H, p->D, L.Dp};
  lstm_seq_strip_values(a, s);
  HIPCHK(hipGetLastError());
  return LHW_OK;
}

// The actor as the resident rollout's in-wave LSTM step reads it (lhw_humanoid_rollout.hip: lstm_policy_step): [in][out] copies of
// W1cat, W2cat and Wout made here, everything else pointers into theta and the handle's own actor state.
extern "C" int lhw_rnn_rollout_policy(LhwRnn* p, const float* theta, const float* obs_mean, const float* obs_std, uint64_t seed, uint32_t counter,
                                      int deterministic, LhwRolloutLstmPolicy* out, void* stream) {
  if (!p || !theta || !obs_mean || !obs_std || !out) return lhw_fail(LHW_ERR_ARG, "null argument");
  const LstmLayout& L = p->la;
  if (L.H != 256 || L.Dp > 64 || L.O > 16 || L.Op > 16)
    return lhw_fail(LHW_ERR_UNSUPPORTED, "lhw_rnn_rollout_policy: the in-wave LSTM step covers hidden width 256 (this actor: %d), padded observation width <= 64, "
                                         "act_dim <= 16", L.H);
  HIPCHK(hipSetDevice(p->device));
  const size_t H = L.H, n1 = (size_t)L.K1 * 4 * H, n2 = 2 * H * 4 * H;
  if (!p->wt_roll && !(p->wt_roll = p->mem.get_lazy<float>(n1 + n2 + H * L.Op)))
    return lhw_fail(LHW_ERR_HIP, "lhw_rnn_rollout_policy: allocation of the transposed weights failed");
  const float* th = theta + p->off_actor;
  float *w1t = p->wt_roll, *w2t = w1t + n1, *wot = w2t + n2;
  const LhwTransposeJob jobs[3] = {{th + L.w1, w1t, 4 * L.H, L.K1, L.K1, 4 * L.H}, {th + L.w2, w2t, 4 * L.H, 2 * L.H, 2 * L.H, 4 * L.H}, {th + L.wo, wot, L.O, L.H, L.H, L.Op}};
  lhw_transpose3(jobs, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  out->w1t = w1t; out->bi1 = th + L.bi1; out->bh1 = th + L.bh1;
  out->w2t = w2t; out->bi2 = th + L.bi2; out->bh2 = th + L.bh2;
  out->wot = wot; out->bo = th + L.bo;
  out->stdv = theta + p->off_std; out->obs_mean = obs_mean; out->obs_std = obs_std;
  out->h1 = p->rxh1[0] + L.Dp; out->h1_ld = L.K1;
  out->h2 = p->rxh2[0] + L.H; out->h2_ld = 2 * L.H;
  out->c1 = p->rc1[0]; out->c2 = p->rc2[0];
  out->state_rows = p->Nroll;
  out->obs_dim = p->D; out->obs_pad = L.Dp; out->act_dim = L.O; out->act_pad = L.Op; out->hidden = L.H;
  out->deterministic = deterministic; out->seed = seed; out->counter = counter;
  return LHW_OK;
}

// BPTT over one minibatch of B env columns of the time-major rollout ([T][N] buffers; xn / xm = normalised (mirrored)
// observations [T*N][Dp], done = LHW_DONE_* flags).  Accumulates into grad and stats_dev[0..5] like lhw_ppo_grad.
extern "C" int lhw_rnn_grad(LhwRnn* p, const float* theta, float* grad, int32_t T, int32_t N, const float* xn, const float* xm,
                            const float* act, const float* old_logp, const float* adv, const float* ret, const uint8_t* done,
                            const int32_t* cols, int32_t B, float* stats_dev, void* stream) {
  if (!p || !theta || !grad || !xn || !act || !old_logp || !adv || !ret || !done || !cols || !stats_dev) return lhw_fail(LHW_ERR_ARG, "null argument");
  if (T <= 0 || T > p->T || B <= 0 || B > p->Bmax || N <= 0) return lhw_fail(LHW_ERR_ARG, "sequence minibatch %d x %d exceeds capacity %d x %d", T, B, p->T, p->Bmax);
  const int mir = p->use_mirror && xm != nullptr;
  HIPCHK(hipSetDevice(p->device));
  hipStream_t s = (hipStream_t)stream;
  const int Dp = p->la.Dp, K1 = p->la.K1, Op = p->la.Op;
  const int Bt = mir ? 2 * B : B, R = T * B;
  p->wa.Bt = Bt; p->wc.Bt = B;
  unsigned char *reset_a = p->reset, *reset_c = p->reset + (size_t)2 * p->T * p->Bmax;
  const size_t n = (size_t)R * Dp;
  hipLaunchKernelGGL(seq_gather_kernel, dim3((n + 255) / 256), dim3(256), 0, s, cols, T, N, B, Bt, Dp, K1, p->A, xn, mir ? xm : (const float*)nullptr,
                     act, old_logp, adv, ret, done, p->wa.xh1, p->wc.xh1, p->mb_act, p->mb_logp, p->mb_adv, p->mb_ret, reset_a, reset_c);
  const float *th_a = theta + p->off_actor, *th_c = theta + p->off_critic;
  // Whole-sequence strips: each network's forward time loop and BPTT time loop are one launch each; a slab of 32 rows occupies one CU for the whole
  // sequence, so the critic's launches run on the side stream beside the actor's.  Everything that accumulates into grad or uses the shared
  // split-K scratch stays on `s` in the order of the other path: the same seed gives the same bits on either path.
  const bool fused = p->seq_fused && p->wt_seq[0] && p->wt_seq[1] && p->side;
  p->last_grad_fused = fused ? 1 : 0;
  const StreamPair sp{s, fused ? p->side : s, p->ev_fork, p->ev_join};
  hipStream_t sc = sp.sc;
  const float *wt_a = fused ? p->wt_seq[0] : nullptr, *wt_c = fused ? p->wt_seq[1] : nullptr;
  sp.fork();
  if (fused) {
    lstm_seq_strip_prepare(th_c + p->lc.w1, th_c + p->lc.w2, p->H, Dp, p->wt_seq[1], sc);
    lstm_seq_strip_prepare(th_a + p->la.w1, th_a + p->la.w2, p->H, Dp, p->wt_seq[0], s);
  }
  lstm_seq_forward(p->la, th_a, p->wa, T, reset_a, s, wt_a);
  lstm_seq_forward(p->lc, th_c, p->wc, T, reset_c, sc, wt_c);
  sp.join();
  const int nblk = (R + 255) / 256;
  // the loss kernel writes d loss / d read-out for the normal rows (and the mirrored rows); rows it does not own stay zero
  HIPCHK(hipMemsetAsync(p->wa.dy, 0, sizeof(float) * (size_t)T * Bt * Op, s));
  hipLaunchKernelGGL(ppo_loss_kernel, dim3(nblk), dim3(256), 0, s, R, 0, p->A, Op, p->wa.y, p->wc.y, p->mb_act, p->mb_logp, p->mb_adv,
                     p->mb_ret, theta + p->off_std, p->clip, p->mirror_coeff, mir, p->d_act_src, p->d_act_sign, p->wa.dy, p->wc.dy,
                     p->learn_std ? p->dstd : (float*)nullptr, p->stats_part, (const float*)nullptr, (const unsigned char*)nullptr, 0.f, 0.f,
                     mir ? B : 0, 1.f);
  hipLaunchKernelGGL(reduce_rows_kernel, dim3(1), dim3(64), 0, s, p->stats_part, nblk, NSTAT, stats_dev);
  if (p->learn_std) {
    colsum_det(p->dstd, R, Op, p->A, grad + p->off_std, p->part, s);
    hipLaunchKernelGGL(entropy_grad_kernel, dim3(1), dim3(64), 0, s, theta + p->off_std, p->A, p->ent_coeff, grad + p->off_std);
  }
  const int kc = 2048;
  sp.fork();
  lstm_seq_bptt(p->lc, th_c, p->wc, T, reset_c, sc, wt_c);
  lstm_seq_bptt(p->la, th_a, p->wa, T, reset_a, s, wt_a);
  lstm_seq_wgrad(p->la, grad + p->off_actor, p->wa, T, p->part, kc, s);
  sp.join();
  lstm_seq_wgrad(p->lc, grad + p->off_critic, p->wc, T, p->part, kc, s);
  HIPCHK(hipGetLastError());
  return LHW_OK;
}

extern "C" int lhw_rnn_apply(LhwRnn* p, float* theta, float* grad, float* adam_m, float* adam_v, int64_t step, float grad_scale,
                             void* stream) {
  return learner_apply(p, theta, grad, adam_m, adam_v, step, grad_scale, stream);
}
extern "C" int lhw_rnn_debug_grad_sqnorms(LhwRnn* p, float* out2_host) { return learner_grad_sqnorms(p, out2_host); }
extern "C" int lhw_rnn_normalize(LhwRnn* p, const float* obs, int64_t R, const float* obs_mean, const float* obs_std, float* xn,
                                 float* xm, void* stream) {
  return learner_normalize(p, obs, R, obs_mean, obs_std, xn, xm, stream);
}
