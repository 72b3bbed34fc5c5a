// The resident rollout: policy step + control step for T control steps of a rollout in ONE launch, wave by wave.
//
// Takes over the body of the reference's worker loop (rl/workers/rollout_worker.py:142-181: `action = policy(state)`,
// `env.step(action)`, store, reset on episode end) for every env of a range.  In the reference each worker advances its own
// env without ever waiting for another one; the launch-per-control-step pipeline (lhw_env_step_range + lhw_ppo_forward_at)
// instead ends every control step on the slowest of the batch's wavefronts before the policy launch -- a launch lasts as long
// as its slowest wave (1.58x the mean wave of a 4096-env launch) and the chip drains meanwhile.  Here a wavefront keeps its
// env(s) for the whole rollout and evaluates the actor itself:
//
//   for t in 0 .. T-1:   obs[t] rows of the wave's envs  ->  policy_step  ->  act[t], logp[t]
//                        control_step<0, TASK, W>         ->  obs[t+1], term_obs[t], rew[t], done[t]   (auto-reset inside)
//
// The policy step is the fused strip launch of lhw_mlp_strip.hip restated for the 1-2 rows a wave owns: two rows x 256 hidden
// units are nowhere near an MFMA tile (1/16 of a 32x32 tile), so the layers are plain v_fma_f32 over all 64 lanes -- lane l
// owns hidden units 4l .. 4l+3 of both rows, the weights come straight from L2 in [in][out] order (one 16-byte load per lane
// and k row = 1 KB per wave, fully coalesced; 0.3 MB per wave and control step, ~2 % of a control step), the activations sit
// in the stepper's LDS stage region, which is dead between control steps.  Every value is produced by the SAME operations in
// the SAME order as mlp_fwd_strip_kernel's (normalisation expression, fmaf chains over ascending k from 0, bias added after
// the chain, the read-out cut into eight 32-k partial sums added in ascending order, lhw_policy_sample), so a rollout collected
// here is bitwise the rollout of the launch-per-step pipeline (tests/test_rollout_resident*.py).
//
// Two envs per wave (W = 32): an env that exceeds the layout's 8 contacts in a control step returns untouched from
// control_step<0, TASK, 32>; the launch-per-step path repeats its step with the one-env-per-wave kernel in a second launch.
// Here the wave does that itself, at once: both envs have left the LDS working set by then (everything persistent is in the HBM
// record between control steps), so the wave re-interprets its LDS allocation as the W = 64 layout and runs
// control_step<0, TASK, 64> for the flagged env with all 64 lanes -- same code, same bits as the second launch.
#define LHW_SUBSTEP_PRIO 1   // the sub-steps of these kernels alternate the wave's issue priority with its SIMD partner's (substep(), lhw_humanoid_dev.h)
#include "lhw_humanoid_dev.h"
#include "lhw_lstm_cell.h"
#include "lhw_policy.h"

#define PH 256      // hidden width of the actor (rl/policies/actor.py:127)
#define PKQ 32      // the read-out is summed as PH / PKQ partial products of PKQ k each (SKQ of lhw_mlp_strip.hip)
#define PXK 64      // capacity of the padded observation row
#define PO_MAX 16   // action dims the read-out's lane mapping covers (JVRC 12, H1 10): four column groups of four
#define PXC 256     // columns of the padded observation row the history family's step holds in LDS at a time (policy_step_wide's chunk): a multiple of 2 PU
#define PXW LHW_ROLLOUT_HISTORY_MAX_OBS_PAD   // widest padded observation row the history family takes: a validated limit (PXW / PXC chunks), not an LDS size

// agent-scope loads / stores of the job queue's progress words (a wave on another XCD wrote them: not through this XCD's L2)
#if defined(__HIP_EMU__)
__device__ __forceinline__ unsigned lhw_load_agent(const unsigned* p) { return *p; }
__device__ __forceinline__ void lhw_store_agent(unsigned* p, unsigned v) { *p = v; }
#else
__device__ __forceinline__ unsigned lhw_load_agent(const unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void lhw_store_agent(unsigned* p, unsigned v) { __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT); }
#endif

template <class POL>
struct HRolloutT {
  int T;                 // control steps of this launch
  int n_total;           // envs of the batch: row count of one time slice of the buffers below
  float* obs;            // [T + 1][n_total][obs_dim]: slice 0 is read (the observation to act on first), 1 .. T are written
  float* act;            // [T][n_total][act_dim]
  float* logp;           // [T][n_total]
  float* tob;            // [T][n_total][obs_dim] observation returned by env.step itself (bootstrap input where an episode ended)
  float* rew;            // [T][n_total]
  unsigned char* done;   // [T][n_total] LHW_DONE_* flags
  float* rew_terms;      // [n_total][n_terms] of the last control step, nullable
  // Job queue (nullable = off: wave b of the grid keeps env group b for all T steps).  When the range has more env groups than the
  // chip has wave slots, a group's rollout is cut into jobs of `chunk` control steps; the resident waves pop jobs from queue[0]
  // in the order (chunk 0 of every group, chunk 1 of every group, ...), queue[1 + group] counts the group's finished chunks.
  unsigned* queue;
  int chunk;
  long long tin_step;    // doubles per control step of the task-input export (n_total * LHW_TASK_INPUT_DIM), 0: the per-launch record (or none);
                         // the stepping task's second record (HState::stin) follows it at LHW_STEP_TASK_INPUT_DIM doubles per env
  POL pol;
};
// Policy kinds of the resident rollout: the feed-forward 256-256 actor (policy_step) and the two-cell LSTM actor (lstm_policy_step).  The kind
// is a template parameter of rollout_steps and picks the kernel's argument struct, so a feed-forward kernel holds nothing of the LSTM step.
// POLICY_HIST: the feed-forward actor on an observation HISTORY (obs_history_len > 1: rows of history_len x base width, policy_step_wide).
// (the enum is lhw_internal.h's: the API layer names the kind of a request)
struct LstmPolicyArg {
  LhwRolloutLstmPolicy q;
  const unsigned char* reset0;   // [n_total] rows whose episode starts with the rollout's first observation (their state counts as zero)
};
struct HistPolicyArg {
  LhwRolloutPolicy q;    // obs_dim = history_len x the env's base width
  float *base, *tbase;   // [n_total][base width] each: what control_step writes (observation / terminal observation of the step); history_shift reads them
};
typedef HRolloutT<LhwRolloutPolicy> HRollout;
typedef HRolloutT<LstmPolicyArg> HRolloutLstm;
typedef HRolloutT<HistPolicyArg> HRolloutHist;
template <int PK> struct RolloutOf { typedef HRollout type; };
template <> struct RolloutOf<POLICY_LSTM> { typedef HRolloutLstm type; };
template <> struct RolloutOf<POLICY_HIST> { typedef HRolloutHist type; };

// One 256-wide ReLU layer for the wave's G rows: hout[r][n] = relu(chain_k fmaf(W^T[k][n], xin[r][k]) + bias[n]), n = 4 wl .. 4 wl + 3.
// The weight rows of PU consecutive k are requested as one batch of independent 16-byte loads, a batch ahead of the one being
// multiplied (left to itself the compiler waits for every load right behind its issue -- s_waitcnt vmcnt(0) 293 times per policy
// step, each a full L2 round trip; the scheduling barriers keep the batches apart, as in slab_mma of lhw_mlp_strip.hip).  Rows
// k >= K are clamped copies of row K - 1 multiplied by the zeros xin holds there (K is padded to a multiple of 2 PU by the caller's
// buffer: the observation row is zero beyond its width up to PXK), so the prefetches run past the end unconditionally.
#define PU 8
// HALF: fp16 operands (BASELINE config 5) -- every weight and every activation is rounded to fp16 before it is multiplied (the product of
// two fp16 values is exact in float32), the sums stay float32 over ascending k; biases, the ReLU and the read-out's final sum are float32.
#if defined(__HIP_EMU__)
__device__ __forceinline__ float r16(float x) { return emu_f16_round(x); }
#else
__device__ __forceinline__ float r16(float x) { return (float)(_Float16)x; }
#endif
template <int G, bool HALF>
__device__ __forceinline__ void policy_hidden(const float* __restrict__ wt, const float* __restrict__ bias, const float* xin, const int ldx, const int K,
                                              float* hout, const int wl) {
  float acc[G][4];
#pragma unroll
  for (int r = 0; r < G; r++)
#pragma unroll
    for (int c = 0; c < 4; c++) acc[r][c] = 0.f;
  const float4* w4 = reinterpret_cast<const float4*>(wt) + wl;
  float4 wa[PU], wb[PU];
  auto load = [&](float4 (&w)[PU], const int k0) {
#pragma unroll
    for (int j = 0; j < PU; j++) w[j] = w4[(size_t)min(k0 + j, K - 1) * (PH / 4)];
  };
  auto mul = [&](const float4 (&w)[PU], const int k0) {
#pragma unroll
    for (int j = 0; j < PU; j++)
#pragma unroll
      for (int r = 0; r < G; r++) {
        const float x = xin[r * ldx + k0 + j];   // (HALF: rounded when it was stored)
        const float w0 = HALF ? r16(w[j].x) : w[j].x, w1 = HALF ? r16(w[j].y) : w[j].y, w2 = HALF ? r16(w[j].z) : w[j].z, w3 = HALF ? r16(w[j].w) : w[j].w;
        acc[r][0] = fmaf(w0, x, acc[r][0]); acc[r][1] = fmaf(w1, x, acc[r][1]);
        acc[r][2] = fmaf(w2, x, acc[r][2]); acc[r][3] = fmaf(w3, x, acc[r][3]);
      }
  };
  load(wa, 0);
  for (int k0 = 0; k0 < K; k0 += 2 * PU) {
    load(wb, k0 + PU);
    __builtin_amdgcn_sched_barrier(0);
    mul(wa, k0);
    __builtin_amdgcn_sched_barrier(0);
    load(wa, k0 + 2 * PU);
    __builtin_amdgcn_sched_barrier(0);
    if (k0 + PU < K) mul(wb, k0 + PU);
    __builtin_amdgcn_sched_barrier(0);
  }
  const float4 b = reinterpret_cast<const float4*>(bias)[wl];
#pragma unroll
  for (int r = 0; r < G; r++) {
    float4 v = make_float4(fmaxf(acc[r][0] + b.x, 0.f), fmaxf(acc[r][1] + b.y, 0.f), fmaxf(acc[r][2] + b.z, 0.f), fmaxf(acc[r][3] + b.w, 0.f));
    if (HALF) v = make_float4(r16(v.x), r16(v.y), r16(v.z), r16(v.w));   // the next layer's operand
    *reinterpret_cast<float4*>(hout + r * PH + 4 * wl) = v;
  }
}

// floats of LDS the policy step of a wave with G rows needs
template <int G> struct PolicyLds { static constexpr int XS = 0, H1 = XS + G * PXK, H2 = H1 + G * PH, PP = H2 + G * PH, TM = PP + 8 * G * 16, FLOATS = TM + G * 16; };

// Actor forward + Gaussian head for the wave's rows (envs env0 .. env0 + nlive - 1 of this time slice); all 64 lanes take part.
template <int G, bool HALF>
__device__ __forceinline__ void policy_step(const LhwRolloutPolicy& q, float* sc, const float* __restrict__ obs_t, float* __restrict__ act_t,
                                            float* __restrict__ logp_t, const int env0, const int nlive, const unsigned genv0, const unsigned counter) {
  typedef PolicyLds<G> PL;
  const int wl = fresh_wave_lane();
  const int D = q.obs_dim, O = q.act_dim, Op = q.act_pad;
  float *xs = sc + PL::XS, *h1 = sc + PL::H1, *h2 = sc + PL::H2, *Pp = sc + PL::PP, *Tm = sc + PL::TM;
  // the normalised observation rows (the expression of stage_input / normalize_kernel), zero beyond the observation width
  for (int i = wl; i < G * PXK; i += 64) {
    const int r = i / PXK, k = i - r * PXK;
    float v = 0.f;
    if (k < D && r < nlive) v = (obs_t[(size_t)(env0 + r) * D + k] - q.obs_mean[k]) / q.obs_std[k];
    xs[i] = HALF ? r16(v) : v;
  }
  SYNC();
  policy_hidden<G, HALF>(q.w1t, q.b1, xs, PXK, q.obs_pad, h1, wl);
  SYNC();
#ifdef LHW_DBG_POL
  if (wl == 0 && env0 == 0) printf("dbg counter %u xs %g %g %g %g h1 %g %g %g %g w1t %g %g b1 %g\n", counter, xs[0], xs[1], xs[36], xs[37], h1[0], h1[1], h1[2], h1[255], q.w1t[0], q.w1t[1], q.b1[0]);
#endif
  policy_hidden<G, HALF>(q.w2t, q.b2, h1, PH, PH, h2, wl);
  SYNC();
  // read-out: lane = (partial q8 of 8, row r, column group cg of four output units); with one row per wave the r = 1 lanes repeat
  // the r = 0 lanes' work and keep it to themselves.  One 16-byte weight load per lane and k (W3^T rows are act_pad floats), PU of
  // them in flight
  const int q8 = wl >> 3, r = (wl >> 2) & 1, rr_ = G == 2 ? r : 0, cg = wl & 3;
  const bool colsin = 4 * cg < Op;      // (act_pad = 12: the fourth column group has no columns)
  float pacc[4] = {0.f, 0.f, 0.f, 0.f};
  const float* w3 = q.w3t + (size_t)(q8 * PKQ) * Op + 4 * (colsin ? cg : 0);
  for (int kk0 = 0; kk0 < PKQ; kk0 += PU) {
    float4 w[PU];
#pragma unroll
    for (int j = 0; j < PU; j++) w[j] = *reinterpret_cast<const float4*>(w3 + (size_t)(kk0 + j) * Op);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < PU; j++) {
      const float h = h2[rr_ * PH + q8 * PKQ + kk0 + j];
      const float w0 = HALF ? r16(w[j].x) : w[j].x, w1 = HALF ? r16(w[j].y) : w[j].y, w2 = HALF ? r16(w[j].z) : w[j].z, w3 = HALF ? r16(w[j].w) : w[j].w;
      pacc[0] = fmaf(h, 4 * cg + 0 < O ? w0 : 0.f, pacc[0]); pacc[1] = fmaf(h, 4 * cg + 1 < O ? w1 : 0.f, pacc[1]);
      pacc[2] = fmaf(h, 4 * cg + 2 < O ? w2 : 0.f, pacc[2]); pacc[3] = fmaf(h, 4 * cg + 3 < O ? w3 : 0.f, pacc[3]);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  if (colsin && (G == 2 || r == 0)) {
#pragma unroll
    for (int c = 0; c < 4; c++) Pp[(q8 * G + rr_) * 16 + 4 * cg + c] = pacc[c];
  }
  SYNC();
  if (wl < 16 * G) {
    const int rr = wl >> 4, col = wl & 15;
    if (col < O && rr < nlive) {
      float s = Pp[rr * 16 + col];
#pragma unroll
      for (int j = 1; j < PH / PKQ; j++) s += Pp[(j * G + rr) * 16 + col];
      s += q.b3[col];
      float term;
      const float a = lhw_policy_sample(s, q.stdv[col], q.seed, genv0 + (unsigned)rr, counter, col, q.deterministic, &term);
      act_t[(size_t)(env0 + rr) * O + col] = a;
      Tm[rr * 16 + col] = term;
    }
  }
  SYNC();
  if (wl < nlive) {
    float lp = 0.f;
    for (int k = 0; k < O; k++) lp += Tm[wl * 16 + k];     // (the order of sample_kernel's sum)
    logp_t[env0 + wl] = lp;
  }
  SYNC();
}

// ------------------------------------------------------------------------------------------------ observation history
// obs_history_len > 1 (reference envs/common/base_humanoid_env.py:53,177-197,274): the observation is the last H base observations, newest
// first, H x OBS wide.  Rows wider than the strip kernel's 64 columns go through the per-layer GEMMs in the launch-per-step pipeline
// (mlp_forward, lhw_ppo.hip), so the in-wave step follows THAT path's order: hidden layers as policy_hidden (one fmaf chain over
// ascending k from +0, bias, ReLU -- what gemm_f32_kernel computes), the read-out ONE chain over k = 0 .. 255 with the bias after it,
// as lstm_policy_step's.  LDS: the rows (XK floats each), h1, h2, the Gaussian head's terms -- no partial sums.
template <int G, int XK> struct PolicyLdsWide { static constexpr int XS = 0, H1 = XS + G * XK, H2 = H1 + G * PH, TM = H2 + G * PH, FLOATS = TM + G * 16; };
template <int PK, int G> struct PolicyLdsOf { static constexpr int FLOATS = PolicyLds<G>::FLOATS; };
template <int G> struct PolicyLdsOf<POLICY_HIST, G> { static constexpr int FLOATS = PolicyLdsWide<G, PXC>::FLOATS; };

// policy_hidden in two parts, so that a unit's chain can run over more than one piece of a row: policy_hidden_acc continues the lane's chains
// (acc) over rows 0 .. K - 1 of wt and the K values of each xin row -- the load batches, the clamped rows past K and the order of policy_hidden --
// and policy_hidden_out adds the bias, applies the ReLU and stores.  acc from +0, one policy_hidden_acc, policy_hidden_out IS policy_hidden.
// A restatement beside it and not its new body: built from these two parts, policy_hidden compiled to other code in the kernels of the plain
// family (118 instructions more in the two-envs-per-wave kernels, the same resource figures), which are to stay the kernels without the feature.
template <int G, bool HALF>
__device__ __forceinline__ void policy_hidden_acc(float (&acc)[G][4], const float* __restrict__ wt, const float* xin, const int ldx, const int K, const int wl) {
  const float4* w4 = reinterpret_cast<const float4*>(wt) + wl;
  float4 wa[PU], wb[PU];
  auto load = [&](float4 (&w)[PU], const int k0) {
#pragma unroll
    for (int j = 0; j < PU; j++) w[j] = w4[(size_t)min(k0 + j, K - 1) * (PH / 4)];
  };
  auto mul = [&](const float4 (&w)[PU], const int k0) {
#pragma unroll
    for (int j = 0; j < PU; j++)
#pragma unroll
      for (int r = 0; r < G; r++) {
        const float x = xin[r * ldx + k0 + j];   // (HALF: rounded when it was stored)
        const float w0 = HALF ? r16(w[j].x) : w[j].x, w1 = HALF ? r16(w[j].y) : w[j].y, w2 = HALF ? r16(w[j].z) : w[j].z, w3 = HALF ? r16(w[j].w) : w[j].w;
        acc[r][0] = fmaf(w0, x, acc[r][0]); acc[r][1] = fmaf(w1, x, acc[r][1]);
        acc[r][2] = fmaf(w2, x, acc[r][2]); acc[r][3] = fmaf(w3, x, acc[r][3]);
      }
  };
  load(wa, 0);
  for (int k0 = 0; k0 < K; k0 += 2 * PU) {
    load(wb, k0 + PU);
    __builtin_amdgcn_sched_barrier(0);
    mul(wa, k0);
    __builtin_amdgcn_sched_barrier(0);
    load(wa, k0 + 2 * PU);
    __builtin_amdgcn_sched_barrier(0);
    if (k0 + PU < K) mul(wb, k0 + PU);
    __builtin_amdgcn_sched_barrier(0);
  }
}
template <int G, bool HALF>
__device__ __forceinline__ void policy_hidden_out(const float (&acc)[G][4], const float* __restrict__ bias, float* hout, const int wl) {
  const float4 b = reinterpret_cast<const float4*>(bias)[wl];
#pragma unroll
  for (int r = 0; r < G; r++) {
    float4 v = make_float4(fmaxf(acc[r][0] + b.x, 0.f), fmaxf(acc[r][1] + b.y, 0.f), fmaxf(acc[r][2] + b.z, 0.f), fmaxf(acc[r][3] + b.w, 0.f));
    if (HALF) v = make_float4(r16(v.x), r16(v.y), r16(v.z), r16(v.w));   // the next layer's operand
    *reinterpret_cast<float4*>(hout + r * PH + 4 * wl) = v;
  }
}

template <int G, bool HALF, int XK>
__device__ __forceinline__ void policy_step_wide(const LhwRolloutPolicy& q, float* sc, const float* __restrict__ obs_t, float* __restrict__ act_t,
                                                 float* __restrict__ logp_t, const int env0, const int nlive, const unsigned genv0, const unsigned counter) {
  typedef PolicyLdsWide<G, XK> PL;
  static_assert(XK % (2 * PU) == 0, "policy_hidden multiplies batches of 2 PU rows");
  const int wl = fresh_wave_lane();
  const int D = q.obs_dim, O = q.act_dim, Op = q.act_pad;
  float *xs = sc + PL::XS, *h1 = sc + PL::H1, *h2 = sc + PL::H2, *Tm = sc + PL::TM;
  // Layer 1 over the row in chunks of XK columns: xs holds one chunk at a time, the lane's chains (acc) run on from chunk to chunk -- for
  // every width the one ascending-k chain from +0 -- and the bias and the ReLU come behind the last one.  A row of up to XK columns is one trip.
  float acc[G][4];
#pragma unroll
  for (int r = 0; r < G; r++)
#pragma unroll
    for (int c = 0; c < 4; c++) acc[r][c] = 0.f;
  for (int c0 = 0; c0 < q.obs_pad; c0 += XK) {
    const int kc = min(XK, q.obs_pad - c0);                // columns of this chunk
    const int KP = (kc + 2 * PU - 1) & ~(2 * PU - 1);      // (what policy_hidden_acc's batches read: zero beyond the observation width)
#pragma unroll
    for (int r = 0; r < G; r++)
      for (int k = wl; k < KP; k += 64) {      // (the expression of normalize_kernel)
        const int col = c0 + k;
        float v = 0.f;
        if (col < D && r < nlive) v = (obs_t[(size_t)(env0 + r) * D + col] - q.obs_mean[col]) / q.obs_std[col];
        xs[r * XK + k] = HALF ? r16(v) : v;
      }
    SYNC();
    policy_hidden_acc<G, HALF>(acc, q.w1t + (size_t)c0 * PH, xs, XK, kc, wl);
    if (c0 + XK < q.obs_pad) SYNC();      // every lane has read this chunk before the next one takes its place
  }
  policy_hidden_out<G, HALF>(acc, q.b1, h1, wl);
  SYNC();
  policy_hidden<G, HALF>(q.w2t, q.b2, h1, PH, PH, h2, wl);
  SYNC();
  // read-out: lane = (row, output unit), one chain over k = 0 .. 255 from +0 and the bias after it, 16 weight loads in flight
  if (wl < 16 * G) {
    const int rr = wl >> 4, col = wl & 15;
    if (col < O && rr < nlive) {
      const float* w = q.w3t + col;
      float s = 0.f;
      for (int k0 = 0; k0 < PH; k0 += 16) {
        float wv[16];
#pragma unroll
        for (int j = 0; j < 16; j++) wv[j] = w[(size_t)(k0 + j) * Op];
#pragma unroll
        for (int j = 0; j < 16; j++) s = fmaf(h2[rr * PH + k0 + j], HALF ? r16(wv[j]) : wv[j], s);
      }
      s += q.b3[col];
      float term;
      const float a = lhw_policy_sample(s, q.stdv[col], q.seed, genv0 + (unsigned)rr, counter, col, q.deterministic, &term);
      act_t[(size_t)(env0 + rr) * O + col] = a;
      Tm[rr * 16 + col] = term;
    }
  }
  SYNC();
  if (wl < nlive) {
    float lp = 0.f;
    for (int k = 0; k < O; k++) lp += Tm[wl * 16 + k];     // (the order of sample_kernel's sum)
    logp_t[env0 + wl] = lp;
  }
  SYNC();
}

// The history rows of the wave's live envs behind control step t (batched_env.history_update, base_humanoid_env.py:177-197): the base
// observation the step returned in front of the previous full observation without its oldest entry -- zeros (+0) instead where the episode
// ended and the env was reset (the deque is emptied and zero-filled); the terminal row keeps the history the episode ended with.
//   obs[t+1][env] = [ base      | done ? 0 : obs[t][env][0 : D - OBS] ]
//   tob[t][env]   = [ term base | obs[t][env][0 : D - OBS] ]
// Nothing of the history lives in the wave or in the env record: obs[t] is the state, so the job queue needs nothing more.  All 64 lanes.
__device__ __forceinline__ void history_shift(const HistPolicyArg& hp, const int OBS, const float* obs_t, float* obs_n, float* tob_t, const unsigned char* done_t,
                                              const int env0, const int nlive) {
  const int wl = fresh_wave_lane();
  const int D = hp.q.obs_dim;
  for (int r = 0; r < nlive; r++) {
    const size_t env = (size_t)(env0 + r);
    const bool ended = done_t[env] != 0;
    for (int i = wl; i < D; i += 64) {
      float o, tb;
      if (i < OBS) {
        o = hp.base[env * OBS + i];
        tb = hp.tbase[env * OBS + i];
      } else {
        tb = obs_t[env * D + i - OBS];
        o = ended ? 0.f : tb;
      }
      obs_n[env * D + i] = o;
      tob_t[env * D + i] = tb;
    }
  }
}

// ------------------------------------------------------------------------------------------------ LSTM actor
// Gaussian_LSTM_Actor (rl/policies/actor.py:191-286: two stacked LSTMCells of 256 units and a linear read-out) for the wave's G rows, as
// lhw_rnn_forward evaluates it per control step (lhw_rnn.hip): the same values bit for bit, so a resident rollout and a launch-per-step
// rollout can follow each other on the same LhwRnn handle.  Lane l owns hidden units 4l .. 4l + 3 of all FOUR gates of both rows: per
// row k of a transposed weight matrix ([in][4 x 256], gate-major columns) four 16-byte loads per lane, each gate's 1 KB coalesced; the
// cell update and the cell state are then lane-local.  Every gate pre-activation is ONE fmaf chain over ascending k from +0 over the
// concatenated input [x | h_prev] -- what gemm_f32_kernel's v_mfma_f32_32x32x2_f32 loop computes -- followed by lhw_lstm_cell.
// LPU weight rows (4 LPU loads per lane) are requested a batch ahead of the one being multiplied, as in policy_hidden: 32 accumulators
// and two batches of 16 LPU registers.  LPU = 2: with 4 the two-envs-per-wave kernels spill 6 - 8 VGPRs where their feed-forward twins spill none.
#ifndef LPU
#define LPU 2
#endif
template <int G>
__device__ __forceinline__ void lstm_gates(float (&acc)[G][4][4], const float* __restrict__ wt, const int K, const float* xin, const int ldx, const int wl) {
  const float4* w4 = reinterpret_cast<const float4*>(wt) + wl;      // (a weight row is 4 PH floats = PH float4)
  float4 wa[LPU][4], wb[LPU][4];
  auto load = [&](float4 (&w)[LPU][4], const int k0) {
#pragma unroll
    for (int j = 0; j < LPU; j++)
#pragma unroll
      for (int g = 0; g < 4; g++) w[j][g] = w4[(size_t)min(k0 + j, K - 1) * PH + g * (PH / 4)];
  };
  auto mul = [&](const float4 (&w)[LPU][4], const int k0) {
#pragma unroll
    for (int j = 0; j < LPU; j++)
#pragma unroll
      for (int r = 0; r < G; r++) {
        const float x = xin[r * ldx + k0 + j];
#pragma unroll
        for (int g = 0; g < 4; g++) {
          acc[r][g][0] = fmaf(w[j][g].x, x, acc[r][g][0]); acc[r][g][1] = fmaf(w[j][g].y, x, acc[r][g][1]);
          acc[r][g][2] = fmaf(w[j][g].z, x, acc[r][g][2]); acc[r][g][3] = fmaf(w[j][g].w, x, acc[r][g][3]);
        }
      }
  };
  load(wa, 0);      // (K is a multiple of LPU; the loads past the end are clamped copies of the last row and are not multiplied)
  for (int k0 = 0; k0 < K; k0 += 2 * LPU) {
    load(wb, k0 + LPU);
    __builtin_amdgcn_sched_barrier(0);
    mul(wa, k0);
    __builtin_amdgcn_sched_barrier(0);
    load(wa, k0 + 2 * LPU);
    __builtin_amdgcn_sched_barrier(0);
    if (k0 + LPU < K) mul(wb, k0 + LPU);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// The cell update of the lane's four units for every live row: reads and writes the cell state in HBM (c, [rows][PH]), writes the new
// hidden state to its HBM slot (hs, row stride ld) and returns it in hnew (zero for rows beyond nlive).
template <int G>
__device__ __forceinline__ void lstm_cells(const float (&acc)[G][4][4], const float* __restrict__ bi, const float* __restrict__ bh, float* c, float* hs, const int ld,
                                           const bool (&rst)[G], const int env0, const int nlive, const int wl, float (&hnew)[G][4]) {
  float b_ih[4][4], b_hh[4][4];      // [unit][gate]
#pragma unroll
  for (int g = 0; g < 4; g++) {
    const float4 a = reinterpret_cast<const float4*>(bi)[g * (PH / 4) + wl], b = reinterpret_cast<const float4*>(bh)[g * (PH / 4) + wl];
    b_ih[0][g] = a.x; b_ih[1][g] = a.y; b_ih[2][g] = a.z; b_ih[3][g] = a.w;
    b_hh[0][g] = b.x; b_hh[1][g] = b.y; b_hh[2][g] = b.z; b_hh[3][g] = b.w;
  }
#pragma unroll
  for (int r = 0; r < G; r++) {
#pragma unroll
    for (int u = 0; u < 4; u++) hnew[r][u] = 0.f;
    if (r < nlive) {
      float4* crow = reinterpret_cast<float4*>(c + (size_t)(env0 + r) * PH) + wl;
      const float4 c4 = rst[r] ? make_float4(0.f, 0.f, 0.f, 0.f) : *crow;
      const float cp[4] = {c4.x, c4.y, c4.z, c4.w};
      float cn[4], gt[4];
#pragma unroll
      for (int u = 0; u < 4; u++) hnew[r][u] = lhw_lstm_cell(acc[r][0][u], acc[r][1][u], acc[r][2][u], acc[r][3][u], b_ih[u], b_hh[u], cp[u], gt, &cn[u]);
      *crow = make_float4(cn[0], cn[1], cn[2], cn[3]);
      *reinterpret_cast<float4*>(hs + (size_t)(env0 + r) * ld + 4 * wl) = make_float4(hnew[r][0], hnew[r][1], hnew[r][2], hnew[r][3]);
    }
  }
}

// LSTM actor forward + Gaussian head for the wave's rows; all 64 lanes take part.  rst_t [n_total]: rows whose episode starts with this
// observation (the rollout's reset0 at its first step, the previous step's done flags afterwards) -- their stored state counts as zero,
// which is what rnn_reset_kernel does to it in front of lhw_rnn_forward's GEMMs.  LDS as PolicyLds<G>: xs, h1 (the previous hidden state,
// overwritten by the new one once layer 1 is done), h2 likewise, the Gaussian head's terms.
template <int G>
__device__ __forceinline__ void lstm_policy_step(const LhwRolloutLstmPolicy& q, float* sc, const float* __restrict__ obs_t, float* __restrict__ act_t,
                                                 float* __restrict__ logp_t, const unsigned char* rst_t, const int env0, const int nlive, const unsigned genv0,
                                                 const unsigned counter) {
  typedef PolicyLds<G> PL;
  const int wl = fresh_wave_lane();
  const int D = q.obs_dim, O = q.act_dim, Op = q.act_pad, Dp = q.obs_pad;
  float *xs = sc + PL::XS, *h1 = sc + PL::H1, *h2 = sc + PL::H2, *Tm = sc + PL::TM;
  bool rst[G];
#pragma unroll
  for (int r = 0; r < G; r++) rst[r] = r < nlive && rst_t[env0 + r] != 0;
  for (int i = wl; i < G * PXK; i += 64) {      // (the expression of normalize_ld_kernel, zero beyond the observation width)
    const int r = i / PXK, k = i - r * PXK;
    float v = 0.f;
    if (k < D && r < nlive) v = (obs_t[(size_t)(env0 + r) * D + k] - q.obs_mean[k]) / q.obs_std[k];
    xs[i] = v;
  }
  for (int i = wl; i < G * PH; i += 64) {
    const int r = i / PH, k = i - r * PH;
    const bool keep = r < nlive && !rst[r];
    h1[i] = keep ? q.h1[(size_t)(env0 + r) * q.h1_ld + k] : 0.f;
    h2[i] = keep ? q.h2[(size_t)(env0 + r) * q.h2_ld + k] : 0.f;
  }
  SYNC();
  float acc[G][4][4], hn[G][4];
  auto zero = [&]() {
#pragma unroll
    for (int r = 0; r < G; r++)
#pragma unroll
      for (int g = 0; g < 4; g++)
#pragma unroll
        for (int u = 0; u < 4; u++) acc[r][g][u] = 0.f;
  };
  auto put = [&](float* h) {
#pragma unroll
    for (int r = 0; r < G; r++) *reinterpret_cast<float4*>(h + r * PH + 4 * wl) = make_float4(hn[r][0], hn[r][1], hn[r][2], hn[r][3]);
  };
  // cell 1 over [x | h1_prev]: rows 0 .. Dp - 1 of W1cat^T, then its 256 recurrent rows
  zero();
  lstm_gates<G>(acc, q.w1t, Dp, xs, PXK, wl);
  lstm_gates<G>(acc, q.w1t + (size_t)Dp * 4 * PH, PH, h1, PH, wl);
  lstm_cells<G>(acc, q.bi1, q.bh1, q.c1, q.h1, q.h1_ld, rst, env0, nlive, wl, hn);
  SYNC();      // every lane has read the previous h1
  put(h1);
  SYNC();
  // cell 2 over [h1 | h2_prev]
  zero();
  lstm_gates<G>(acc, q.w2t, PH, h1, PH, wl);
  lstm_gates<G>(acc, q.w2t + (size_t)PH * 4 * PH, PH, h2, PH, wl);
  lstm_cells<G>(acc, q.bi2, q.bh2, q.c2, q.h2, q.h2_ld, rst, env0, nlive, wl, hn);
  SYNC();
  put(h2);
  SYNC();
  // read-out: lane = (row, output unit), ONE chain over k = 0 .. 255 from +0 and the bias after it (the read-out GEMM of lhw_rnn_forward;
  // not the eight partial sums of policy_step, which mirror the strip kernel), 16 weight loads in flight
  if (wl < 16 * G) {
    const int rr = wl >> 4, col = wl & 15;
    if (col < O && rr < nlive) {
      const float* w = q.wot + col;
      float s = 0.f;
      for (int k0 = 0; k0 < PH; k0 += 16) {
        float wv[16];
#pragma unroll
        for (int j = 0; j < 16; j++) wv[j] = w[(size_t)(k0 + j) * Op];
#pragma unroll
        for (int j = 0; j < 16; j++) s = fmaf(h2[rr * PH + k0 + j], wv[j], s);
      }
      s += q.bo[col];
      float term;
      const float a = lhw_policy_sample(s, q.stdv[col], q.seed, genv0 + (unsigned)rr, counter, col, q.deterministic, &term);
      act_t[(size_t)(env0 + rr) * O + col] = a;
      Tm[rr * 16 + col] = term;
    }
  }
  SYNC();
  if (wl < nlive) {
    float lp = 0.f;
    for (int k = 0; k < O; k++) lp += Tm[wl * 16 + k];     // (the order of sample_kernel's sum)
    logp_t[env0 + wl] = lp;
  }
  SYNC();
}

// Control steps [t0, t1) of env group `grp` of the range (the G envs one wave advances together).
template <int TASK, int W, bool STATS, bool DIAG, int PK, bool ACT = false>
__device__ __forceinline__ void rollout_steps(HModelRef m, HParamsRef p, const HLaunch& lz, const HState& st, const typename RolloutOf<PK>::type& ro, unsigned char* SGraw, int grp,
                                              int t0, int t1) {
  using L = typename LayoutOf<TASK, W>::type;
  using L1 = typename LayoutOf<TASK, 64>::type;
  constexpr int G = 64 / W;   // envs per wavefront
  L* SG = reinterpret_cast<L*>(SGraw);
  const int eidx0 = grp * G;
  const int nlive = min(G, lz.env_count - eidx0);
  const int env0 = lz.env_first + eidx0;
  const int OBS = humanoid_base_obs_dim(TASK);
  const size_t N = (size_t)ro.n_total;
  // (diagnostic, lhw_env_debug_wave_cycles, DIAG instantiations only: shader-clock cycles the group's control steps took, summed over the
  //  rollout's chunks; control_step leaves the last step's own figure in the same word, so the running sum is picked up before the chunk's
  //  first step)
  WaveClock<DIAG> wc, wc_before;
  if constexpr (DIAG) {
    wc_before.t = 0;
    if (st.wave_cyc && t0 > 0) {
      const int wl = fresh_wave_lane();
      if ((wl & (W - 1)) == 0 && (W == 32 ? (wl >> 5) : 0) < nlive) wc_before.t = st.wave_cyc[env0 + (W == 32 ? (wl >> 5) : 0)];
    }
    wc.t = st.wave_cyc ? (long long)clock64() : 0;
  }
  for (int t = t0; t < t1; t++) {
    GROUP_SYNC(64);
    // what this wave wrote in the previous control step (the observation rows it now reads; after a W = 64 re-run, by other
    // lanes than the ones that read them) is visible
    __threadfence();
    const float* obs_t = ro.obs + (size_t)t * N * OBS;
    if constexpr (PK == POLICY_HIST) obs_t = ro.obs + (size_t)t * N * (size_t)ro.pol.q.obs_dim;   // (a time slice holds rows of history_len x OBS)
    float* act_t = ro.act + (size_t)t * N * m.nu;
    if constexpr (PK == POLICY_LSTM) {
      // (the flags of the step before: read here, at the start of the policy step, so they also hold where the job queue cut the rollout)
      const unsigned char* rst_t = t == 0 ? ro.pol.reset0 : ro.done + (size_t)(t - 1) * N;
      lstm_policy_step<G>(ro.pol.q, reinterpret_cast<float*>(SG[0].U), obs_t, act_t, ro.logp + (size_t)t * N, rst_t, env0, nlive, p.env_id_base + (unsigned)env0,
                          ro.pol.q.counter + (unsigned)t);
#ifdef LHW_RO_POLICY2X   // (analysis builds only: the second call advances the state once more -- a timing, not a rollout)
      lstm_policy_step<G>(ro.pol.q, reinterpret_cast<float*>(SG[0].U), obs_t, act_t, ro.logp + (size_t)t * N, rst_t, env0, nlive, p.env_id_base + (unsigned)env0,
                          ro.pol.q.counter + (unsigned)t);
#endif
    } else if constexpr (PK == POLICY_HIST) {
      if (ro.pol.q.fp16_operands)
        policy_step_wide<G, true, PXC>(ro.pol.q, reinterpret_cast<float*>(SG[0].U), obs_t, act_t, ro.logp + (size_t)t * N, env0, nlive, p.env_id_base + (unsigned)env0,
                                       ro.pol.q.counter + (unsigned)t);
      else
        policy_step_wide<G, false, PXC>(ro.pol.q, reinterpret_cast<float*>(SG[0].U), obs_t, act_t, ro.logp + (size_t)t * N, env0, nlive, p.env_id_base + (unsigned)env0,
                                        ro.pol.q.counter + (unsigned)t);
    } else {
      if (ro.pol.fp16_operands)
        policy_step<G, true>(ro.pol, reinterpret_cast<float*>(SG[0].U), obs_t, act_t, ro.logp + (size_t)t * N, env0, nlive, p.env_id_base + (unsigned)env0,
                             ro.pol.counter + (unsigned)t);
      else
        policy_step<G, false>(ro.pol, reinterpret_cast<float*>(SG[0].U), obs_t, act_t, ro.logp + (size_t)t * N, env0, nlive, p.env_id_base + (unsigned)env0,
                              ro.pol.counter + (unsigned)t);
#ifdef LHW_RO_POLICY2X   // (analysis builds: the policy step twice -- the difference in rollout time is its cost)
      policy_step<G, false>(ro.pol, reinterpret_cast<float*>(SG[0].U), obs_t, act_t, ro.logp + (size_t)t * N, env0, nlive, p.env_id_base + (unsigned)env0,
                            ro.pol.counter + (unsigned)t);
#endif
    }
    __threadfence();   // the action rows are read back by the lanes of their env's group
    const int wl = fresh_wave_lane();
    const int g = W == 32 ? (wl >> 5) : 0, lane = wl & (W - 1);
    float* obs_n = ro.obs + (size_t)(t + 1) * N * OBS;
    float* tob_t = ro.tob + (size_t)t * N * OBS;
    if constexpr (PK == POLICY_HIST) {   // control_step writes rows of OBS floats: the per-env base rows, which history_shift puts in front of the history
      obs_n = ro.pol.base;
      tob_t = ro.pol.tbase;
    }
    float* rew_t = ro.rew + (size_t)t * N;
    unsigned char* done_t = ro.done + (size_t)t * N;
    bool ovf = false;
    HLaunch lzt = lz;
    lzt.tin_off = (long long)t * ro.tin_step;   // (the batched sim facade of EVERY control step, for reward-only task plug-ins: lhw_env_rollout_task_inputs)
    if (g < nlive)
      ovf = control_step<0, TASK, W, STATS, DIAG, ACT>(m, p, lzt, st, SG, SG[g], env0 + g, lane, act_t, obs_n, tob_t, rew_t, done_t, ro.rew_terms, nullptr, nullptr);
#ifndef LHW_RO_NO_RERUN   // (analysis builds: without the in-wave re-run, to see what its code costs the hot path -- nothing measurable)
    if constexpr (W == 32) {
      GROUP_SYNC(64);
      const unsigned long long ob = __ballot(ovf);
      if (ob) {
        HLaunch lz1 = lzt;
        lz1.only_flagged = 1;   // (store_record clears the env's flag and counts the re-run)
        L1* S1 = reinterpret_cast<L1*>(SGraw);
        for (int gg = 0; gg < 2; gg++)
          if ((ob >> (32 * gg)) & 1ull) {
            SYNC();
            // (as a call -- it is rare -- the kernel spills 12 fewer VGPRs and 200 fewer SGPRs and is 9 % SLOWER: profiles/r05_calls_and_scratch.txt)
            control_step<0, TASK, 64, STATS, DIAG, ACT>(m, p, lz1, st, S1, S1[0], env0 + gg, fresh_wave_lane(), act_t, obs_n, tob_t, rew_t, done_t, ro.rew_terms, nullptr, nullptr);
          }
      }
    }
#endif
    if constexpr (PK == POLICY_HIST) {
      GROUP_SYNC(64);
      __threadfence();   // the base rows and the flag of this control step (after a W = 64 re-run written by other lanes than the ones that read them)
      const size_t DH = (size_t)ro.pol.q.obs_dim;
      history_shift(ro.pol, OBS, obs_t, ro.obs + (size_t)(t + 1) * N * DH, ro.tob + (size_t)t * N * DH, done_t, env0, nlive);
      // (the rows are published to the next policy step -- in queue mode another wave's -- by the fences that publish obs[t + 1] without a
      //  history: the one at the top of the loop, and the one behind the chunk in the job loop)
    }
  }
  if constexpr (DIAG) {
    if (st.wave_cyc) {
      const int wl = fresh_wave_lane();
      const int g = W == 32 ? (wl >> 5) : 0;
      if ((wl & (W - 1)) == 0 && g < nlive) st.wave_cyc[env0 + g] = wc_before.t + ((long long)clock64() - wc.t);
    }
  }
}

// QUEUE = false: wave b of the grid keeps env group b for all T control steps.
// QUEUE = true: the grid is the chip's resident set of waves and drains a job list (HRollout::queue) -- a group whose envs are slow
// (stepping task: the walking mode and the terrain under the feet set the contact count for a whole episode; the waves of one
// launch spread +-20 % around their mean, and with two groups per wave slot the launch ends 22 % after the mean slot) no longer
// decides when its slot's NEXT group can start: the slot takes whatever job is next.  Nothing of an env lives in the wave between
// control steps (control_step reads the HBM record and writes it back), so which wave runs a job does not matter to the bits.
// A separate instantiation: wrapped into the job loop, the two-envs-per-wave kernels spill 25 more VGPRs and lose 2.8 % (round 5,
// same box, jvrc_walk @ 4096), and at 8192 envs their waves are within +-2 % of each other anyway (queue +0.1 %).
// Kernel families from one text (each once more for the LSTM actor, policy kind POLICY_LSTM, and for the observation history, POLICY_HIST): humanoid_rollout_kernel, and humanoid_rollout_stats_kernel, which also keeps the per-term episode
// statistics (control_step<.., STATS>) and is launched instead while lhw_env_enable_term_stats is in force.  Generated by a macro and not
// through a shared device function, so that the plain family stays, instruction for instruction, the kernels without the feature.
#define DEFINE_ROLLOUT_KERNEL(NAME, STATS, DIAG, PK, ACT) \
template <int TASK, int W, bool QUEUE>                                                                                                                              \
__global__ void __launch_bounds__(64, LHW_WAVES_PER_SIMD) NAME(const HDevBlock* __restrict__ bp, HLaunch lz, HState st, typename RolloutOf<PK>::type ro) {                          \
  using L = typename LayoutOf<TASK, W>::type;                                                                                                                       \
  using L1 = typename LayoutOf<TASK, 64>::type;                                                                                                                     \
  constexpr int G = 64 / W;                                                                                                                                         \
  constexpr size_t LDS_BYTES = sizeof(L) * G > sizeof(L1) ? sizeof(L) * G : sizeof(L1);                                                                             \
  static_assert(W == 64 || sizeof(L1) <= sizeof(L) * G, "the one-env-per-wave layout must fit the wave's two-env allocation (8 workgroups per CU)");                \
  static_assert(L::USIZE_ * 2 - 48 >= PolicyLdsOf<PK, G>::FLOATS, "the policy step's activations must fit the stage region in front of the observation staging");         \
  __shared__ __attribute__((aligned(16))) unsigned char SGraw[LDS_BYTES];                                                                                           \
  LHW_LDS_POISON(SGraw);                                                                                                                                            \
  HParamsRef p = LHW_BLOCK_PARAMS(bp);                                                                                                                              \
  HModelRef m = LHW_BLOCK_MODEL(bp);                                                                                                                                \
  const int n_groups = (lz.env_count + G - 1) / G;                                                                                                                  \
  if constexpr (!QUEUE) {                                                                                                                                           \
    if ((int)blockIdx.x >= n_groups) return;                                                                                                                        \
    rollout_steps<TASK, W, STATS, DIAG, PK, ACT>(m, p, lz, st, ro, SGraw, (int)blockIdx.x, 0, ro.T);                                                                          \
  } else {                                                                                                                                                          \
    const int n_chunks = (ro.T + ro.chunk - 1) / ro.chunk;                                                                                                          \
    for (;;) {                                                                                                                                                      \
      unsigned j = 0;                                                                                                                                               \
      if (fresh_wave_lane() == 0) j = atomicAdd(ro.queue, 1u);                                                                                                      \
      j = (unsigned)__builtin_amdgcn_readlane((int)j, 0);                                                                                                           \
      if (j >= (unsigned)n_groups * (unsigned)n_chunks) break;                                                                                                      \
      const int c = (int)(j / (unsigned)n_groups), grp = (int)(j % (unsigned)n_groups);                                                                             \
      const int t0 = c * ro.chunk, t1 = min(ro.T, t0 + ro.chunk);                                                                                                   \
      /* the group's previous chunk was popped n_groups - 1 jobs ago by a wave that is running: it ends without waiting for anyone */                               \
      while (lhw_load_agent(ro.queue + 1 + grp) < (unsigned)c) __builtin_amdgcn_s_sleep(32);                                                                        \
      rollout_steps<TASK, W, STATS, DIAG, PK, ACT>(m, p, lz, st, ro, SGraw, grp, t0, t1);                                                                                     \
      __threadfence();   /* the group's records, observations and flags of this chunk, before the chunk counts as done */                                           \
      if (fresh_wave_lane() == 0) lhw_store_agent(ro.queue + 1 + grp, (unsigned)(c + 1));                                                                           \
    }                                                                                                                                                               \
  }                                                                                                                                                                 \
}
DEFINE_ROLLOUT_KERNEL(humanoid_rollout_kernel, false, false, POLICY_MLP, false)
DEFINE_ROLLOUT_KERNEL(humanoid_rollout_stats_kernel, true, false, POLICY_MLP, false)
// ... and with the diagnostic clocks (control_step<.., DIAG>, rollout_steps' wave clock), launched instead while one of them is armed.  The
// plain feed-forward family only: with a clock armed, a rollout of any other family is declined (humanoid_rollout, include/lhw.h)
DEFINE_ROLLOUT_KERNEL(humanoid_rollout_diag_kernel, false, true, POLICY_MLP, false)
// the same two families with the LSTM actor's in-wave step (lhw_env_rollout_lstm)
DEFINE_ROLLOUT_KERNEL(humanoid_rollout_lstm_kernel, false, false, POLICY_LSTM, false)
DEFINE_ROLLOUT_KERNEL(humanoid_rollout_lstm_stats_kernel, true, false, POLICY_LSTM, false)
// ... and with the feed-forward actor on an observation history (lhw_env_rollout_history, history_len > 1): rows of up to PXW columns
DEFINE_ROLLOUT_KERNEL(humanoid_rollout_hist_kernel, false, false, POLICY_HIST, false)
DEFINE_ROLLOUT_KERNEL(humanoid_rollout_hist_stats_kernel, true, false, POLICY_HIST, false)
// ... and, behind all of them, the feed-forward family with the actuator randomisation (control_step<.., ACT>), without and with the term
// statistics, launched instead while lhw_env_set_actuator_randomization has armed it.  The other policy kinds and the clocks have no such
// kernels: their rollouts are declined while it is armed (humanoid_rollout, include/lhw.h)
DEFINE_ROLLOUT_KERNEL(humanoid_rollout_act_kernel, false, false, POLICY_MLP, true)
DEFINE_ROLLOUT_KERNEL(humanoid_rollout_act_stats_kernel, true, false, POLICY_MLP, true)

// ------------------------------------------------------------------------------------------------ host side
// A policy kind's kernel families -- plain, with the term statistics, with the diagnostic clocks, with the actuator randomisation without and
// with the statistics (the last three of the feed-forward kind only: the other kinds' cells stay empty) -- : the one place that names them.  The launch tables below are built from it, so a kernel is instantiated where a table
// names it and nowhere else.  FAMILY: a table's first index.
enum { FAMILY_PLAIN = 0, FAMILY_STATS = 1, FAMILY_DIAG = 2, FAMILY_ACT = 3, FAMILY_ACT_STATS = 4, FAMILY_COUNT = 5 };
template <int PK> using RolloutFn = void (*)(const HDevBlock*, HLaunch, HState, typename RolloutOf<PK>::type);
template <int PK, int FAMILY, int TASK, int W, bool QUEUE>
constexpr RolloutFn<PK> rollout_kernel() {
  constexpr bool STATS = FAMILY == FAMILY_STATS;
#if defined(LHW_ONLY_WALK) && !defined(LHW_ROLLOUT_STEP_TU)   // (development builds: this unit compiles the jvrc_walk kernels only, the other tasks' cells stay empty)
  if constexpr (TASK != TASK_WALK) return nullptr; else
#endif
  if constexpr (FAMILY == FAMILY_DIAG) {
    if constexpr (PK == POLICY_MLP) return humanoid_rollout_diag_kernel<TASK, W, QUEUE>; else return nullptr;
  } else if constexpr (FAMILY == FAMILY_ACT) {
    if constexpr (PK == POLICY_MLP) return humanoid_rollout_act_kernel<TASK, W, QUEUE>; else return nullptr;
  } else if constexpr (FAMILY == FAMILY_ACT_STATS) {
    if constexpr (PK == POLICY_MLP) return humanoid_rollout_act_stats_kernel<TASK, W, QUEUE>; else return nullptr;
  } else if constexpr (PK == POLICY_LSTM) {
    if constexpr (STATS) return humanoid_rollout_lstm_stats_kernel<TASK, W, QUEUE>; else return humanoid_rollout_lstm_kernel<TASK, W, QUEUE>;
  } else if constexpr (PK == POLICY_HIST) {
    if constexpr (STATS) return humanoid_rollout_hist_stats_kernel<TASK, W, QUEUE>; else return humanoid_rollout_hist_kernel<TASK, W, QUEUE>;
  } else {
    if constexpr (STATS) return humanoid_rollout_stats_kernel<TASK, W, QUEUE>; else return humanoid_rollout_kernel<TASK, W, QUEUE>;
  }
}

// The stepping task's two instantiations live in a translation unit of their own, lhw_humanoid_rollout_step.hip (this file included with
// LHW_ROLLOUT_STEP_TU defined): it is compiled with LLVM's iterative ILP scheduling strategy, which makes the one-env-per-wave kernels 3 % faster
// (the two-envs-per-wave kernels are built with iterative-maxocc instead: _lib.EXTRA_FLAGS, profiles/r06_stepper_compiler_flags.txt) -- and the two
// halves compile in parallel.
template <int PK>
void humanoid_rollout_launch_step(int family, bool queued, dim3 grid, hipStream_t s, const HDevBlock* b_dev, HLaunch lz, HState st,
                                  const typename RolloutOf<PK>::type& ro);
#ifdef LHW_ROLLOUT_STEP_TU
template <int PK>
void humanoid_rollout_launch_step(int family, bool queued, dim3 grid, hipStream_t s, const HDevBlock* b_dev, HLaunch lz, HState st,
                                  const typename RolloutOf<PK>::type& ro) {
  // [family][not queued].  The plain family is named first, and the kinds are instantiated below in the order MLP, LSTM, HIST: the compiler
  // emits kernels in the order it meets them, and theirs is then the order without the feature
  static constexpr RolloutFn<PK> table[FAMILY_COUNT][2] = {{rollout_kernel<PK, FAMILY_PLAIN, TASK_STEP, 64, true>(), rollout_kernel<PK, FAMILY_PLAIN, TASK_STEP, 64, false>()},
                                                           {rollout_kernel<PK, FAMILY_STATS, TASK_STEP, 64, true>(), rollout_kernel<PK, FAMILY_STATS, TASK_STEP, 64, false>()},
                                                           {rollout_kernel<PK, FAMILY_DIAG, TASK_STEP, 64, true>(), rollout_kernel<PK, FAMILY_DIAG, TASK_STEP, 64, false>()},
                                                           {rollout_kernel<PK, FAMILY_ACT, TASK_STEP, 64, true>(), rollout_kernel<PK, FAMILY_ACT, TASK_STEP, 64, false>()},
                                                           {rollout_kernel<PK, FAMILY_ACT_STATS, TASK_STEP, 64, true>(), rollout_kernel<PK, FAMILY_ACT_STATS, TASK_STEP, 64, false>()}};
  const RolloutFn<PK> k = table[family][!queued];
  if (k) hipLaunchKernelGGL(k, grid, dim3(64), 0, s, b_dev, lz, st, ro);   // (an empty cell: humanoid_rollout has declined the request)
}
#define ROLLOUT_STEP_KIND(PK) \
  template void humanoid_rollout_launch_step<PK>(int, bool, dim3, hipStream_t, const HDevBlock*, HLaunch, HState, const typename RolloutOf<PK>::type&);
ROLLOUT_STEP_KIND(POLICY_MLP) ROLLOUT_STEP_KIND(POLICY_LSTM) ROLLOUT_STEP_KIND(POLICY_HIST)
#else
int humanoid_last_rollout_queued(const HumanoidEnv* h) { return h->last_rollout_queued; }

// the two-envs-per-wave launches of one policy kind
template <int PK>
static void rollout_launch_fast(HumanoidEnv* h, int family, dim3 grid, hipStream_t s, const HLaunch& lz, const HState& st, const typename RolloutOf<PK>::type& ro) {
  // [family][task: walk, h1_walk, stand].  The plain family is named first: the compiler emits kernels in the order it meets them, and
  // theirs is then the order without the feature
  static constexpr RolloutFn<PK> table[FAMILY_COUNT][3] = {
      {rollout_kernel<PK, FAMILY_PLAIN, TASK_WALK, 32, false>(), rollout_kernel<PK, FAMILY_PLAIN, TASK_H1WALK, 32, false>(), rollout_kernel<PK, FAMILY_PLAIN, TASK_STAND, 32, false>()},
      {rollout_kernel<PK, FAMILY_STATS, TASK_WALK, 32, false>(), rollout_kernel<PK, FAMILY_STATS, TASK_H1WALK, 32, false>(), rollout_kernel<PK, FAMILY_STATS, TASK_STAND, 32, false>()},
      {rollout_kernel<PK, FAMILY_DIAG, TASK_WALK, 32, false>(), rollout_kernel<PK, FAMILY_DIAG, TASK_H1WALK, 32, false>(), rollout_kernel<PK, FAMILY_DIAG, TASK_STAND, 32, false>()},
      {rollout_kernel<PK, FAMILY_ACT, TASK_WALK, 32, false>(), rollout_kernel<PK, FAMILY_ACT, TASK_H1WALK, 32, false>(), rollout_kernel<PK, FAMILY_ACT, TASK_STAND, 32, false>()},
      {rollout_kernel<PK, FAMILY_ACT_STATS, TASK_WALK, 32, false>(), rollout_kernel<PK, FAMILY_ACT_STATS, TASK_H1WALK, 32, false>(), rollout_kernel<PK, FAMILY_ACT_STATS, TASK_STAND, 32, false>()}};
  const RolloutFn<PK> k = table[family][h->p.task == TASK_WALK ? 0 : (h->p.task == TASK_H1WALK ? 1 : 2)];
  if (k) hipLaunchKernelGGL(k, grid, dim3(64), 0, s, (const HDevBlock*)h->b_dev, lz, st, ro);
}

// everything of a resident rollout but the policy view (ro.pol, filled by the caller) and the checks (humanoid_rollout); -4 HIP error
template <int PK>
static int rollout_launch(HumanoidEnv* h, typename RolloutOf<PK>::type& ro, const HumanoidRollout& rq, hipStream_t s) {
  const int first = rq.first, count = rq.count, T = rq.T;
  ro.T = T; ro.n_total = h->p.n_envs;
  ro.obs = rq.obs; ro.act = rq.act; ro.logp = rq.logp; ro.tob = rq.term_obs; ro.rew = rq.rew; ro.done = rq.done; ro.rew_terms = rq.rew_terms;
  ro.queue = nullptr; ro.chunk = 0;
  ro.tin_step = rq.tin_all ? (long long)h->p.n_envs * LHW_TASK_INPUT_DIM : 0;
  HState st = h->st;
  if (rq.tin_all) {
    st.tin = rq.tin_all;       // [T][n_envs][LHW_TASK_INPUT_DIM]: every control step's record instead of the last one's
    // [T][n_envs][LHW_STEP_TASK_INPUT_DIM] (stepping task, exported together with tin_all: its slice offset follows tin_off), or none
    // (an armed per-launch stepping record is [n_envs] long: not written at the time slices of tin_all)
    st.stin = rq.stin_all;
  }
  const HLaunch lz{first, count, 0, h->iteration, 0};
  // Stepping task with more env groups than wave slots: the resident waves share a job queue of `chunk`-step pieces instead of a
  // group each (humanoid_rollout_kernel<.., QUEUE = true>).  LHW_ROLLOUT_CHUNK: control steps per job (default 10; 0 = one wave per
  // group whatever the batch).  LHW_ROLLOUT_SLOTS: tests only,
  // the number of wave slots to assume (so that a small batch takes the queue path).
  const int n_groups = h->fast ? (count + 1) / 2 : count;
  int grid_n = n_groups;
  {
    const int chunk_env = getenv("LHW_ROLLOUT_CHUNK") ? atoi(getenv("LHW_ROLLOUT_CHUNK")) : 10;
    int slots = getenv("LHW_ROLLOUT_SLOTS") ? atoi(getenv("LHW_ROLLOUT_SLOTS")) : 0;
    if (slots <= 0) {
      static int chip_slots = 0;
      if (!chip_slots) {
        int nb = humanoid_occupancy(), dev = 0;
        hipDeviceProp_t prop;
        if (nb <= 0 || hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return -4;
        chip_slots = nb * prop.multiProcessorCount;
      }
      slots = chip_slots;
    }
    if (!h->fast && chunk_env > 0 && n_groups > slots && T > chunk_env) {
      // two words per env: the ranges of concurrent launches (disjoint by contract) get disjoint pieces
      if (!h->ro_queue && !(h->ro_queue = h->mem.get_lazy<unsigned>((size_t)h->p.n_envs * 2 + 2, LhwDevMem::RAW))) return -4;
      ro.queue = h->ro_queue + 2 * (size_t)first;
      ro.chunk = chunk_env;
      if (hipMemsetAsync(ro.queue, 0, ((size_t)n_groups + 1) * sizeof(unsigned), s) != hipSuccess) return -4;
      grid_n = slots;
    }
  }
  const dim3 grid(grid_n);
  h->last_rollout_queued = ro.queue != nullptr;
  // per-term episode statistics armed: the kernels that keep them; a diagnostic clock armed: the kernels that run it (never both: humanoid_rollout)
  // ... the actuator randomisation armed (no clock is armed then: humanoid_set_actuator_rand): the kernels that carry it, with or without the statistics
  const int family = humanoid_diag_armed(h) ? FAMILY_DIAG
                     : humanoid_act_armed(h) ? (h->p.tstat != nullptr ? FAMILY_ACT_STATS : FAMILY_ACT)
                                             : (h->p.tstat != nullptr ? FAMILY_STATS : FAMILY_PLAIN);
  if (h->fast) rollout_launch_fast<PK>(h, family, grid, s, lz, st, ro);
#ifndef LHW_ONLY_WALK
  else humanoid_rollout_launch_step<PK>(family, ro.queue != nullptr, grid, s, (const HDevBlock*)h->b_dev, lz, st, ro);
#endif
  return 0;
}

// (instantiated here, in the order of the kinds, and not where humanoid_rollout happens to name them first: this line decides the order
//  in which the compiler emits the two-envs-per-wave kernels, the one they have had so far)
#define ROLLOUT_KIND(PK) template int rollout_launch<PK>(HumanoidEnv*, typename RolloutOf<PK>::type&, const HumanoidRollout&, hipStream_t);
ROLLOUT_KIND(POLICY_MLP) ROLLOUT_KIND(POLICY_LSTM) ROLLOUT_KIND(POLICY_HIST)

// the shape clauses the in-wave policy steps share: the width of the env's rows, the capacity of the step's padded observation row (PXK / PXW)
template <class POL>
static bool policy_fits(const POL* q, const HumanoidEnv* h, long long obs_dim, int obs_cap) {
  return q->hidden == PH && q->obs_dim == obs_dim && q->act_dim == h->m.nu && q->act_pad <= PO_MAX && !(q->act_pad & 3) && q->act_pad >= q->act_dim &&
         q->obs_pad >= obs_dim && q->obs_pad <= obs_cap && !(q->obs_pad & 3);
}

int humanoid_rollout(HumanoidEnv* h, const HumanoidRollout& rq, hipStream_t s) {
  if (rq.first < 0 || rq.count <= 0 || rq.first + rq.count > h->p.n_envs || rq.T <= 0 || rq.history_len < 1) return -1;
  if (rq.stin_all && (!rq.tin_all || h->p.task != TASK_STEP)) return -1;
  const int base = humanoid_base_obs_dim(h->p.task);
  const long long obs_dim = (long long)rq.history_len * base;
  if (rq.kind == POLICY_LSTM) {   // ... and the policy's state buffers must hold a row per env of the batch
    const LhwRolloutLstmPolicy* q = rq.lstm;
    if (!policy_fits(q, h, obs_dim, PXK) || q->state_rows < h->p.n_envs || (q->h1_ld & 3) || (q->h2_ld & 3) || q->h1_ld < PH || q->h2_ld < PH) return -2;
  } else if (!policy_fits(rq.mlp, h, obs_dim, rq.kind == POLICY_HIST ? PXW : PXK)) {
    return -2;
  }
  // the diagnostic clocks exist in the plain feed-forward family only: no rollout that would silently record nothing
  if (humanoid_diag_armed(h) && (rq.kind != POLICY_MLP || h->p.tstat)) return -5;
  // ... and the actuator randomisation in the feed-forward family without a history only: no rollout that would silently run the plain PD law
  if (humanoid_act_armed(h) && rq.kind != POLICY_MLP) return -6;
  if (!h->fast && h->p.task != TASK_STEP) return -3;   // a walking / standing model that does not fit the two-envs-per-wave layout (or LHW_ONE_ENV_PER_WAVE): launch-per-step only
  if (rq.kind == POLICY_MLP) {
    HRollout ro;
    ro.pol = *rq.mlp;
    return rollout_launch<POLICY_MLP>(h, ro, rq, s);
  }
  if (rq.kind == POLICY_LSTM) {
    HRolloutLstm ro;
    ro.pol.q = *rq.lstm;
    ro.pol.reset0 = rq.reset0;
    return rollout_launch<POLICY_LSTM>(h, ro, rq, s);
  }
  // the policy reads rows of history_len base observations; control_step writes the step's base rows to two per-env scratch buffers,
  // allocated by the first such rollout
  if (!h->hist_base) {
    float* b = h->mem.get_lazy<float>((size_t)h->p.n_envs * base * 2);
    if (!b) return -4;
    h->hist_base = b;
    h->hist_tbase = b + (size_t)h->p.n_envs * base;
  }
  HRolloutHist ro;
  ro.pol.q = *rq.mlp;
  ro.pol.base = h->hist_base;
  ro.pol.tbase = h->hist_tbase;
  return rollout_launch<POLICY_HIST>(h, ro, rq, s);
}
#endif   // LHW_ROLLOUT_STEP_TU
