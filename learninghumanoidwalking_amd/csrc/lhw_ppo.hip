// On-device feed-forward PPO: actor / critic MLP forward, clipped-surrogate loss + backward.  Takes over the arithmetic of
//   Gaussian_FF_Actor / FF_V forward      (reference rl/policies/actor.py:160-188, critic.py:41-49)
//   PPO.update_actor_critic               (reference rl/algos/ppo.py:299-406)
// The dense kernels are lhw_gemm.hip's and lhw_mlp_strip.hip's; the loss kernels, clip + Adam and the advantage entries lhw_learner.hip's;
// the recurrent learner is lhw_rnn.hip.  Network math is float32 like the reference (ATen fp32).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "lhw_gemm.h"
#include "lhw_learner.h"
#include "lhw_mlp_strip_h.h"

// ------------------------------------------------------------------------------------------- MLP plumbing
// Internal parameter layout of one 3-layer MLP (in D -> H -> H -> O), all float32:
//   W1 [H][Dp]  b1 [H]  W2 [H][H]  b2 [H]  W3 [Op][H]  b3 [Op]      Dp = pad4(D), Op = pad4(O)
// (torch Linear layout [out][in]; padded rows/columns are zero and stay zero under Adam).
struct MlpLayout {
  int D, Dp, H, O, Op;
  size_t w1, b1, w2, b2, w3, b3, total;
};
static MlpLayout mlp_layout(int D, int H, int O) {
  MlpLayout L;
  L.D = D; L.Dp = pad4(D); L.H = H; L.O = O; L.Op = pad4(O);
  size_t o = 0;
  L.w1 = o; o += (size_t)H * L.Dp;
  L.b1 = o; o += H;
  L.w2 = o; o += (size_t)H * H;
  L.b2 = o; o += H;
  L.w3 = o; o += (size_t)L.Op * H;
  L.b3 = o; o += L.Op;
  L.total = o;
  return L;
}
// The [in][out] weight copies the strip kernels multiply by (mlp_strip_wt_floats floats: W1^T, W2^T, W3^T) -- this pair owns their layout:
// the six weight / bias pointers of MlpStripFwd / LhwRolloutPolicy for the copies wt of the network at th, and making wt from th
struct StripWeights { const float *w1t, *b1, *w2t, *b2, *w3t, *b3; };
static StripWeights strip_weights(const MlpLayout& L, const float* wt, const float* th) {
  const float* w2t = wt + (size_t)L.Dp * L.H;
  return {wt, th + L.b1, w2t, th + L.b2, w2t + (size_t)L.H * L.H, th + L.b3};
}
static void strip_h_prepare(const MlpLayout& L, const float* th, _Float16* wh, hipStream_t s) { mlp_strip_h_prepare(th + L.w1, th + L.w2, th + L.w3, L.Dp, L.O, wh, s); }
static void strip_prepare(const MlpLayout& L, const float* th, float* wt, hipStream_t s) { mlp_strip_prepare(th + L.w1, th + L.w2, th + L.w3, L.Dp, L.O, L.Op, wt, s); }
// One network as the passes below see it: its layout, its rows of the minibatch workspace, the strip kernels' weight copies and mask
// bits, and the fp16 copies of the --fp16 update.  Built once by lhw_ppo_create (the fp16 part by lhw_ppo_set_update_dtype).  The actor's
// buffers hold 2 R rows (normal rows, from row R the mirrored rows), the critic's R; a pass takes a RowSpan of them.
struct MlpNet {
  MlpLayout L;
  const float* x = nullptr; int ldx = 0;                  // gathered minibatch inputs [rows][ldx]: one buffer for both networks
  float *h1 = nullptr, *h2 = nullptr, *y = nullptr;       // activations [rows][H] x 2, read-out [rows][Op]
  float *dy = nullptr, *dh2 = nullptr, *dh1 = nullptr;    // d loss / d them
  float* wt = nullptr;                                    // [in][out] weight copies for the strip kernels (shapes they take, narrow or wide)
  unsigned *bits1 = nullptr, *bits2 = nullptr;            // ReLU masks of h1 / h2 as bits, forward strip -> backward strip: a launch whose first row is
                                                          // r uses the words from mlp_strip_bits_words(r) on; NULL: max_rows % 64 != 0
  const _Float16* x_h = nullptr; int ldxh = 0;            // fp16 storage: inputs [rows][ldxh], ldxh = Dp rounded up to 8 (16-byte rows), pad columns zero
  _Float16 *h1_h = nullptr, *h2_h = nullptr, *dh2_h = nullptr, *dh1_h = nullptr;   // [rows][H]
  _Float16* wh = nullptr;                                 // the fp16 strip kernels' weight copies for the update (lhw_ppo_debug_set_strip_fp16 allocates them)
};
struct RowSpan { size_t first; int rows; };
// The handle's switches: every LHW_* variable this file reads, read once, by lhw_ppo_create -- a handle sees the environment it was created
// in (DESIGN.md section 4.2 has the table).  lhw_ppo_debug_set_strip_fused / _wide / _fp16 write the same record.
struct Switches {
  int mlp_strip;                  // LHW_MLP_STRIP: 0 = per-layer GEMMs everywhere, 1 = LDS-resident strip kernels in the update, 2 = in rollout inference
                                  // as well (default: the rollout and the update then evaluate the networks with the same kernel, bit for bit)
  int strip_bits, strip_fused;    // LHW_STRIP_BITS: ReLU masks go from forward to backward strip as bits; LHW_STRIP_FUSED: train strips where the step allows
  int strip_wide;                 // rows wider than 64 columns (an observation history) take the wide strip instantiations (Python layer: LHW_STRIP_WIDE)
  int two_streams, graph, fp16_storage;   // LHW_PPO_TWO_STREAMS: the update's critic chain on its own stream; LHW_PPO_GRAPH: lhw_ppo_step captures and
                                          // replays; LHW_FP16_STORAGE: the --fp16 update keeps its activations as fp16 in HBM (0: rounded per GEMM)
  int strip_fp16;                 // fp16 operands take the fp16 strip kernels where float32 operands take the narrow strips (Python layer: LHW_STRIP_FP16)
};
static Switches read_switches() {
  auto on = [](const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; };
  return {on("LHW_MLP_STRIP", 2), on("LHW_STRIP_BITS", 1) != 0, on("LHW_STRIP_FUSED", 1) != 0, 0, on("LHW_PPO_TWO_STREAMS", 1) != 0,
          on("LHW_PPO_GRAPH", 1) != 0, on("LHW_FP16_STORAGE", 1) != 0, 0};
}
// Which kernels one lhw_ppo_grad call launches (update_plan).  The call and the two passes below read it, and the key of a captured step holds
// it by value: whatever decides a launch is in that key.  fwd_strip / bwd_strip are masks: bit 0 the actor, bit 1 the critic.
struct UpdatePlan {
  int32_t half, hstore;           // fp16 operands (gemm_h_kernel); ... that live as fp16 in the nets' *_h buffers (else rounded while staged)
  int32_t fwd_strip, bwd_strip;   // forward layers as one forward strip launch; activation gradients as one backward strip launch (else GEMMs)
  int32_t train;                  // train strips: ONE launch per network runs forward, loss head and backward layers (no fwd / bwd strip then)
  int32_t bits, wide;             // the forward strips leave the ReLU masks as bits for the backward strips; the strip launches are the wide instantiations
  int32_t streams;                // 2: the critic's chain runs on the side stream
};
// ... and what lhw_ppo_forward[_at] and the rollout bracket do (infer_plan)
struct InferPlan {
  int32_t half, strips, policy_step;     // fp16 operands; forward launches run the forward strip (with half: the fp16 one, else per-layer GEMMs); the one-launch policy step is available
  int32_t critic_copies, actor_copies;   // lhw_ppo_begin_rollout makes the critic's [in][out] copies (forward launches read them); the actor's: the bracket opens
};
// How one network's forward or backward pass runs: named fields, filled from the call's plan
struct MlpPass {
  int half = 0; bool hstore = false;               // as UpdatePlan's
  const float* wt = nullptr;                       // forward: the network's READY [in][out] copies, the forward strip runs; NULL: one GEMM per layer
  const _Float16* wh = nullptr;                    // with half: the network's READY fp16 copies, the fp16 forward strip runs / the fp16 backward strip reads them
  bool keep = false, bits = false;                 // forward strip: h1 / h2 are kept for a backward pass (else they never leave LDS), their masks as bits too
  bool bwd_strip = false, have_dh = false;         // backward: dh2 / dh1 by one backward strip launch (with half: the fp16 one); they are already there (train strip launch)
};
// What a captured step was captured for: buffers and stream, minibatch size, the bits of grad_scale, the plan
struct StepKey {
  const void* ptr[12]; int32_t B; uint32_t gs; UpdatePlan plan;
  bool operator==(const StepKey& o) const { return memcmp(this, &o, sizeof o) == 0; }
};
static_assert(std::has_unique_object_representations_v<StepKey>, "StepKey is compared as bytes");

struct LhwPpo : LearnerCore {
  int max_rows;  // capacity of the minibatch workspace (rows per net)
  _Float16* xb_h = nullptr; int ldxh = 0;   // --fp16 update: fp16 copy of xb [2R][ldxh] (the nets' x_h)
  int infer_half = 0, update_half = 0;      // fp16 operands in rollout inference (lhw_ppo_set_inference_dtype) / in every GEMM of the update (lhw_ppo_set_update_dtype)
  MlpNet a, c;            // actor (2R rows), critic (R rows; read-out [R][4])
  // workspace
  float *xb = nullptr;   // [2R][Dp] gathered minibatch inputs (normal rows, then mirrored rows)
  float *mb_act = nullptr, *mb_logp = nullptr, *mb_adv = nullptr, *mb_ret = nullptr;
  float *part = nullptr;       // split-K partial tiles [max slices][H*H]
  float *dstd = nullptr;       // per-row d loss / d std [R][Op]
  float *wt_inf = nullptr;                  // [in][out] weight copies for the strip kernels beside the update's (a.wt, c.wt): WT_SLOTS pairs (actor, critic) for rollout
                                            // inference, one per eighth of the forward workspace, so that concurrent calls (disjoint row ranges, different streams) do not share one
  float *wt_roll = nullptr;                 // ... and the pair made once per rollout by lhw_ppo_begin_rollout (read-only until end_rollout / apply)
  _Float16 *wh_inf = nullptr, *wh_roll = nullptr;   // the same two sets for the fp16 forward strip (with the nets' wh: one block, lhw_ppo_debug_set_strip_fp16)
  const float* roll_theta = nullptr;        // theta the wt_roll (and wh_roll) copies were made from (NULL: no rollout bracket open)
  const float* imit_target = nullptr; const unsigned char* imit_mask = nullptr;   // imitation term of the NEXT lhw_ppo_grad call (lhw_ppo_set_imitation)
  float imit_coeff = 0.f, imit_inv_count = 0.f;
  float *bwd_part = nullptr;   // split-K partials of the weight / bias gradients: actor (two passes), then critic
  int max_slices = 0;
  // the critic's forward / backward chain runs on its own stream beside the actor's (they share only the gathered inputs and
  // the loss kernel): the load / multiply / store phases of one network's GEMMs overlap the other's
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_head = nullptr;
  Switches sw{};
  float* stat_rows = nullptr;   // [NSTAT][max_rows]: the rows' loss terms the train strip launches leave for ppo_stats_rows_kernel
  UpdatePlan last_plan{};       // the plan of the last lhw_ppo_grad (lhw_ppo_debug_last_grad_fused: its train bit)
  // lhw_ppo_step: the captured optimiser step, the two kernel nodes patched before each launch, and what it was captured for
  hipGraph_t step_graph = nullptr; hipGraphExec_t step_exec = nullptr; hipGraphNode_t node_gather = nullptr, node_adam = nullptr;
  StepKey step_key{};
  ~LhwPpo() {
    (void)hipSetDevice(device);
    if (step_exec) (void)hipGraphExecDestroy(step_exec);
    if (step_graph) (void)hipGraphDestroy(step_graph);
    if (side) { (void)hipStreamSynchronize(side); (void)hipStreamDestroy(side); }
    for (hipEvent_t e : {ev_fork, ev_join, ev_head}) if (e) (void)hipEventDestroy(e);
  }
};
#define WT_SLOTS 8
// An actor whose padded observation row is wider than the narrow strips' 64 columns (an observation history) but within the in-wave policy step
// of lhw_env_rollout_history, which reads [in][out] weight copies (LhwPpo::wt_roll) whatever path the handle's own launches take.  Stated from
// the shape alone.  More shapes than the wide strip instantiations take (LHW_MLP_STRIP_MAX_IN_PAD < LHW_ROLLOUT_HISTORY_MAX_OBS_PAD): past the strips'
// capacity the handle's own launches are per-layer GEMMs whatever the switch says, and only the actor's copy is made
static bool rollout_wide_supported(const MlpLayout& L) {
  return L.H == 256 && L.Dp > 64 && L.Dp <= LHW_ROLLOUT_HISTORY_MAX_OBS_PAD && (L.Dp & 3) == 0 && L.O > 0 && L.O <= 32 && L.Op >= L.O;
}
// the strip kernels take this network: a narrow shape, or a wide one with the switch on
static bool strip_shape(const MlpLayout& L, bool wide_on) {
  return mlp_strip_supported(L.H, L.Dp, L.O, L.Op) || (wide_on && mlp_strip_wide_supported(L.H, L.Dp, L.O, L.Op));
}
static bool strip_h_shape(const MlpLayout& L) { return mlp_strip_h_supported(L.H, L.Dp, L.O, L.Op); }   // the fp16 strip kernels do (narrow only)
static bool train_strip_shape(const MlpLayout& L, int critic, bool wide_on) {
  return mlp_train_strip_supported(L.H, L.Dp, L.O, L.Op, critic) || (wide_on && mlp_train_strip_wide_supported(L.H, L.Dp, L.O, L.Op, critic));
}
// The two plans.  (lhw_ppo_create has allocated what a shape the strips take, narrow or wide, needs: the nets' wt, stat_rows, wt_inf / wt_roll.)  The
// strips are not for shapes they reject (per network), nor for --fp16 unless the fp16 strips are switched on (fp16 storage, narrow shapes: forward and backward
// strip, never train strips or mask bits); train strips not for an armed imitation term either: forward strip (or GEMMs), ppo_loss_kernel, backward
static UpdatePlan update_plan(const LhwPpo* p, bool imitation) {
  const Switches& w = p->sw;
  UpdatePlan u{};
  u.half = p->update_half; u.hstore = u.half && p->xb_h != nullptr;
  auto takes = [&](const MlpLayout& L) { return u.half ? strip_h_shape(L) : strip_shape(L, w.strip_wide); };
  const int nets = w.mlp_strip >= 1 && (!u.half || (u.hstore && w.strip_fp16 && p->a.wh)) ? (takes(p->a.L) ? 1 : 0) | (takes(p->c.L) ? 2 : 0) : 0;
  u.train = nets == 3 && !u.half && w.strip_fused && !imitation && train_strip_shape(p->a.L, 0, w.strip_wide) && train_strip_shape(p->c.L, 1, w.strip_wide);
  u.fwd_strip = u.bwd_strip = u.train ? 0 : nets;
  u.bits = u.fwd_strip && !u.half && p->a.bits1 != nullptr;
  u.wide = nets && !strip_shape(p->c.L, false);
  u.streams = w.two_streams ? 2 : 1;
  return u;
}
static InferPlan infer_plan(const LhwPpo* p) {
  InferPlan i{};
  i.half = p->infer_half;
  i.critic_copies = p->sw.mlp_strip >= 2 && p->wt_roll && strip_shape(p->a.L, p->sw.strip_wide) && strip_shape(p->c.L, p->sw.strip_wide);
  i.policy_step = i.critic_copies && !i.half;
  i.strips = i.policy_step || (i.critic_copies && p->sw.strip_fp16 && p->a.wh && strip_h_shape(p->a.L) && strip_h_shape(p->c.L));   // (fp16: the fp16 forward strip)
  // (a wide-row actor's copies serve lhw_env_rollout_history's in-wave step, whatever the handle's own launches run)
  i.actor_copies = i.critic_copies || (p->wt_roll && rollout_wide_supported(p->a.L));
  return i;
}
// y = mlp(x) for the rows of r
static void mlp_forward(const MlpNet& n, const float* theta, RowSpan r, hipStream_t s, const MlpPass& m) {
  const MlpLayout& L = n.L;
  const int R = r.rows, ldx = n.ldx, half = m.half;
  const size_t H = L.H, r0 = r.first;
  const float* x = n.x + r0 * ldx;
  float *h1 = n.h1 + r0 * H, *h2 = n.h2 + r0 * H, *y = n.y + r0 * L.Op;
  if (m.wt) {   // one launch, h1 / h2 stay in LDS between the layers
    const StripWeights w = strip_weights(L, m.wt, theta);
    MlpStripFwd a{w.w1t, w.b1, w.w2t, w.b2, w.w3t, w.b3, x, ldx, L.Dp, L.O, L.Op, R, m.keep ? h1 : nullptr, m.keep ? h2 : nullptr, y};
    if (m.bits) { a.bits1 = n.bits1 + mlp_strip_bits_words(r0); a.bits2 = n.bits2 + mlp_strip_bits_words(r0); }
    mlp_strip_forward(a, s);
    return;
  }
  const bool hs = m.hstore;
  if (m.wh) {   // fp16 operands, one launch: the update's fp16 rows (h1 / h2 kept as fp16) or inference's float32 rows (nothing kept)
    const MlpStripFwdH a{m.wh, theta + L.b1, theta + L.b2, theta + L.b3, hs ? nullptr : x, ldx,
                         hs ? n.x_h + r0 * n.ldxh : nullptr, n.ldxh, L.Dp, L.O, L.Op, R, hs && m.keep ? n.h1_h + r0 * H : nullptr,
                         hs && m.keep ? n.h2_h + r0 * H : nullptr, y};
    mlp_strip_forward_h(a, s);
    return;
  }
  // one GEMM per layer.  hs (--fp16 update): x / h1 / h2 live in fp16, the weights are rounded while staged, y stays float32 for the loss
  auto F = [](const _Float16* q) { return reinterpret_cast<const float*>(q); };
  const float* in[3] = {hs ? F(n.x_h + r0 * n.ldxh) : x, hs ? F(n.h1_h + r0 * H) : h1, hs ? F(n.h2_h + r0 * H) : h2};
  float* out[3] = {hs ? reinterpret_cast<float*>(n.h1_h + r0 * H) : h1, hs ? reinterpret_cast<float*>(n.h2_h + r0 * H) : h2, y};
  const int ldin[3] = {hs ? n.ldxh : ldx, L.H, L.H}, K[3] = {L.Dp, L.H, L.H}, N[3] = {L.H, L.H, L.O}, ldo[3] = {L.H, L.H, L.Op};
  const size_t w[3] = {L.w1, L.w2, L.w3}, b[3] = {L.b1, L.b2, L.b3};
  for (int l = 0; l < 3; l++) {
    GemmArgs g{};
    g.A = in[l]; g.lda = ldin[l]; g.a_half = hs; g.B = theta + w[l]; g.ldb = K[l]; g.C = out[l]; g.ldc = ldo[l]; g.c_half = hs && l < 2;
    g.M = R; g.N = N[l]; g.K = K[l]; g.bias = theta + b[l]; g.relu = l < 2;
    launch_gemm<true, true>(g, s, 0, 0, half);
  }
}
// Split-K partial regions of one network's parameter gradients ([slices][count] each), reduced by one reduce_segments launch.
// The K dimension of a weight-gradient GEMM is the minibatch: it is cut into slices so that every GEMM puts ~1000 blocks on the
// chip -- 512-row slices for the 256 x 256 layer (16 output tiles), 128-row slices for the skinny first / last layers (4 tiles),
// whose blocks would otherwise sit through 32 dependent load -> multiply steps with nothing else resident to hide them.
#define KC_WIDE 512
#define KC_SKINNY 128
struct BwdParts { float *w3, *w2, *w1, *b3, *b2, *b1; };
struct BwdSlices { int w3 = 0, w2 = 0, w1 = 0; };
static inline int nsl(int rows, int kc) { return (rows + kc - 1) / kc; }
static size_t bwd_parts_floats(const MlpLayout& L, size_t rows, int passes) {
  const size_t ss = (size_t)passes * (nsl((int)rows, KC_SKINNY) + 1), sw = (size_t)passes * (nsl((int)rows, KC_WIDE) + 1);
  return ss * ((size_t)L.Op * L.H + L.Op) + sw * ((size_t)L.H * L.H + L.H) + ss * ((size_t)L.H * L.Dp + L.H);
}
static BwdParts bwd_parts_carve(const MlpLayout& L, size_t rows, int passes, float* base) {
  const size_t ss = (size_t)passes * (nsl((int)rows, KC_SKINNY) + 1), sw = (size_t)passes * (nsl((int)rows, KC_WIDE) + 1);
  BwdParts P;
  P.w3 = base; base += ss * L.Op * L.H;
  P.b3 = base; base += ss * L.Op;
  P.w2 = base; base += sw * L.H * L.H;
  P.b2 = base; base += sw * L.H;
  P.w1 = base; base += ss * L.H * L.Dp;
  P.b1 = base;
  return P;
}
// Back-propagation through one MLP for R rows given dy [R][Op].  The weight-gradient GEMMs (K = R) leave their partial products
// -- and, from the same operand tiles, the bias gradients' partial column sums -- in P behind the z slices an earlier pass
// wrote; mlp_backward_segments then lists them for the ordered reduction into grad.  Every reduction runs in a fixed order
// (same seed -> bitwise identical weights, the property the reference's tests/test_determinism.py checks).
static void mlp_backward(const MlpNet& n, const float* theta, RowSpan r, const BwdParts& P, BwdSlices& z, hipStream_t s, const MlpPass& m) {
  const MlpLayout& L = n.L;
  const int R = r.rows, half = m.half;
  const size_t H = L.H, r0 = r.first;
  const float* dy = n.dy + r0 * L.Op;
  const bool hs = m.hstore;
  // hs (--fp16 update with fp16 storage): the same five GEMMs on the fp16 copies (dy and the weights are float32)
  auto F = [](const _Float16* q) { return reinterpret_cast<const float*>(q); };
  const float *x = hs ? F(n.x_h + r0 * n.ldxh) : n.x + r0 * n.ldx, *h1 = hs ? F(n.h1_h + r0 * H) : n.h1 + r0 * H, *h2 = hs ? F(n.h2_h + r0 * H) : n.h2 + r0 * H;
  float *dh2 = hs ? reinterpret_cast<float*>(n.dh2_h + r0 * H) : n.dh2 + r0 * H, *dh1 = hs ? reinterpret_cast<float*>(n.dh1_h + r0 * H) : n.dh1 + r0 * H;
  const int ldx = hs ? n.ldxh : n.ldx;
  GemmArgs g{};
  // (have_dh: a train strip launch has taken the strip launch's place, so neither it nor the GEMMs below compute dh2 / dh1 again)
  const bool strip = m.have_dh || m.bwd_strip;
  if (m.bwd_strip && half) {   // the same launch with fp16 operands, on the fp16 copies (the plan: only with fp16 storage)
    const MlpStripBwdH a{m.wh, dy, n.h1_h + r0 * H, n.h2_h + r0 * H, L.O, L.Op, R, n.dh2_h + r0 * H, n.dh1_h + r0 * H};
    mlp_strip_backward_h(a, s);
  } else if (m.bwd_strip) {   // dh2 = (dy W3) * (h2 > 0) and dh1 = (dh2 W2) * (h1 > 0) in one launch, the dh2 slab staying in LDS
    MlpStripBwd a{theta + L.w2, theta + L.w3, dy, h1, h2, L.O, L.Op, R, dh2, dh1};
    if (m.bits) { a.bits1 = n.bits1 + mlp_strip_bits_words(r0); a.bits2 = n.bits2 + mlp_strip_bits_words(r0); }
    mlp_strip_backward(a, s);
  }
  // The skinny weight gradients dW1 / db1 / dW3 / db3: one K-streaming launch behind the activation gradients (wgrad_skinny_kernel; its
  // slices are at least KC_SKINNY rows, so they fit the partial regions; it reads float32), or two split-K GEMMs (other widths, fp16 operands)
  const bool fused_skinny = strip && !half && z.w1 == z.w3 && wgrad_skinny_supported(L.H, L.Dp, L.O, L.Op) && ldx >= L.Dp && !(ldx & 3) && fused_skinny_on();
  // dW3 [O][H] = dy^T h2 ; db3 = colsum(dy)
  g.A = dy; g.lda = L.Op; g.B = h2; g.ldb = L.H; g.b_half = hs; g.M = L.O; g.N = L.H; g.K = R;
  g.part = P.w3 + (size_t)z.w3 * L.O * L.H; g.colsum = P.b3 + (size_t)z.w3 * L.O; g.k_chunk = KC_SKINNY;
  if (!fused_skinny) launch_gemm<false, false>(g, s, 1, 0, half);
  // dh2 = (dy W3) * (h2 > 0)
  if (!strip) {
    g = GemmArgs{};
    g.A = dy; g.lda = L.Op; g.B = theta + L.w3; g.ldb = L.H; g.C = dh2; g.ldc = L.H; g.c_half = hs; g.M = R; g.N = L.H; g.K = L.O;
    g.mask = h2; g.ldmask = L.H; g.mask_half = hs;
    launch_gemm<true, false>(g, s, 0, 0, half);
  }
  // dW2 = dh2^T h1 ; db2 = colsum(dh2)
  g = GemmArgs{};
  g.A = dh2; g.lda = L.H; g.a_half = hs; g.B = h1; g.ldb = L.H; g.b_half = hs; g.M = L.H; g.N = L.H; g.K = R;
  g.part = P.w2 + (size_t)z.w2 * L.H * L.H; g.colsum = P.b2 + (size_t)z.w2 * L.H; g.k_chunk = KC_WIDE;
  if (!half && wgrad_wide_supported(L.H) && wgrad_wide_on()) launch_wgrad_wide(dh2, h1, R, KC_WIDE, g.part, g.colsum, s);
  else launch_gemm<false, false>(g, s, 1, 0, half);
  // dh1 = (dh2 W2) * (h1 > 0)
  if (!strip) {
    g = GemmArgs{};
    g.A = dh2; g.lda = L.H; g.a_half = hs; g.B = theta + L.w2; g.ldb = L.H; g.C = dh1; g.ldc = L.H; g.c_half = hs; g.M = R; g.N = L.H; g.K = L.H;
    g.mask = h1; g.ldmask = L.H; g.mask_half = hs;
    launch_gemm<true, false>(g, s, 0, 0, half);
  }
  // dW1 [H][Dp] = dh1^T x ; db1 = colsum(dh1)
  if (fused_skinny) {
    const int kc = wgrad_skinny_chunk(R), ns = nsl(R, kc);
    WgradSkinnyArgs a{dh1, x, dy, h2, ldx, L.Dp, L.O, L.Op, R, kc, P.w1 + (size_t)z.w1 * L.H * L.Dp, P.b1 + (size_t)z.w1 * L.H,
                      P.w3 + (size_t)z.w3 * L.O * L.H, P.b3 + (size_t)z.w3 * L.O};
    launch_wgrad_skinny(a, s);
    z.w3 += ns; z.w2 += nsl(R, KC_WIDE); z.w1 += ns;
    return;
  }
  g = GemmArgs{};
  g.A = dh1; g.lda = L.H; g.a_half = hs; g.B = x; g.ldb = ldx; g.b_half = hs; g.M = L.H; g.N = L.Dp; g.K = R;
  g.part = P.w1 + (size_t)z.w1 * L.H * L.Dp; g.colsum = P.b1 + (size_t)z.w1 * L.H; g.k_chunk = KC_SKINNY;
  launch_gemm<false, false>(g, s, 1, 0, half);
  z.w3 += nsl(R, KC_SKINNY); z.w2 += nsl(R, KC_WIDE); z.w1 += nsl(R, KC_SKINNY);
}
static void mlp_backward_segments(SegList& S, const MlpLayout& L, float* grad, const BwdParts& P, const BwdSlices& z) {
  seg_add(S, P.w3, grad + L.w3, z.w3, L.O, L.H, L.H);
  seg_add(S, P.b3, grad + L.b3, z.w3, L.O, 1, 1);
  seg_add(S, P.w2, grad + L.w2, z.w2, L.H, L.H, L.H);
  seg_add(S, P.b2, grad + L.b2, z.w2, L.H, 1, 1);
  seg_add(S, P.w1, grad + L.w1, z.w1, L.H, L.Dp, L.Dp);
  seg_add(S, P.b1, grad + L.b1, z.w1, L.H, 1, 1);
}
// ------------------------------------------------------------------------------------------- elementwise kernels
// float32 rows [rows][ld] -> fp16 rows [rows][ldh] (ldh >= cols, pad columns zero): the gathered minibatch inputs of the --fp16 update
__global__ void __launch_bounds__(256) rows_to_half_kernel(const float* __restrict__ src, int ld, int cols, size_t rows, _Float16* __restrict__ dst, int ldh) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * (size_t)ldh) return;
  const size_t r = i / ldh;
  const int c = (int)(i - r * ldh);
  dst[i] = c < cols ? (_Float16)src[r * ld + c] : (_Float16)0.f;
}
// gather a minibatch: rows idx[0..B) of xn -> xb[0..B), of xm -> xb[R..R+B) (if mirror), plus act/logp/adv/ret
struct GatherArgs {
  const int* idx; int B, Rcap, Dp, A;
  const float *xn, *xm, *act, *logp, *adv, *ret;
  float *xb, *mact, *mlogp, *madv, *mret;
};
__global__ void gather_kernel(GatherArgs a) {
  const int* __restrict__ idx = a.idx;
  const int B = a.B, Rcap = a.Rcap, Dp = a.Dp, A = a.A;
  const float *__restrict__ xn = a.xn, *__restrict__ xm = a.xm, *__restrict__ act = a.act, *__restrict__ logp = a.logp, *__restrict__ adv = a.adv,
              *__restrict__ ret = a.ret;
  float *__restrict__ xb = a.xb, *__restrict__ mact = a.mact, *__restrict__ mlogp = a.mlogp, *__restrict__ madv = a.madv, *__restrict__ mret = a.mret;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)B * Dp) return;
  int m = (int)(i / Dp), j = (int)(i - (size_t)m * Dp);
  size_t s = (size_t)idx[m];
  xb[(size_t)m * Dp + j] = xn[s * Dp + j];
  if (xm) xb[((size_t)Rcap + m) * Dp + j] = xm[s * Dp + j];
  if (j < A) mact[(size_t)m * A + j] = act[s * A + j];
  if (j == 0) { mlogp[m] = logp[s]; madv[m] = adv[s]; mret[m] = ret[s]; }
}
extern "C" int lhw_ppo_create(const LhwPpoConfig* c, LhwPpo** out) {
  if (const int rc = learner_check(c, (void**)out, c && c->max_rows > 0)) return rc;
  std::unique_ptr<LhwPpo> p(new LhwPpo());
  p->max_rows = c->max_rows; p->sw = read_switches();
  MlpNet &a = p->a, &cr = p->c;
  a.L = mlp_layout(c->obs_dim, c->hidden, c->act_dim);
  cr.L = mlp_layout(c->obs_dim, c->hidden, 1);
  learner_init(*p, c, a.L.total, cr.L.total);
  const size_t R = p->max_rows, Dp = a.L.Dp, H = p->H, Op = a.L.Op;
  LhwDevMem& mem = p->mem;   // (zero-filled blocks; after a failure the calls below return NULL without trying: one check at the end)
  mem.get(&p->xb, 2 * R * Dp); mem.get(&a.h1, 2 * R * H); mem.get(&a.h2, 2 * R * H); mem.get(&a.y, 2 * R * Op);
  mem.get(&cr.h1, R * H); mem.get(&cr.h2, R * H); mem.get(&cr.y, R * 4); mem.get(&a.dy, 2 * R * Op);
  mem.get(&a.dh2, 2 * R * H); mem.get(&a.dh1, 2 * R * H); mem.get(&cr.dy, R * 4); mem.get(&cr.dh2, R * H);
  mem.get(&cr.dh1, R * H); mem.get(&p->mb_act, R * p->A); mem.get(&p->mb_logp, R); mem.get(&p->mb_adv, R);
  mem.get(&p->mb_ret, R); mem.get(&p->stats, 16); mem.get(&p->dstd, R * Op); mem.get(&p->stats_part, ((R + 255) / 256) * NSTAT);
  mem.get(&p->norm_part, 2 * SUMSQ_BLOCKS);
  p->max_slices = (int)((R + 511) / 512);
  mem.get(&p->part, std::max<size_t>((size_t)p->max_slices * H * std::max<size_t>(H, Dp), (size_t)COLSUM_CHUNKS * H));
  mem.get(&p->bwd_part, bwd_parts_floats(p->a.L, R, 2) + bwd_parts_floats(p->c.L, R, 1));
  a.x = cr.x = p->xb; a.ldx = cr.ldx = (int)Dp;
  // (the strip kernels' scratch for every shape they take, narrow or wide: whether a wide shape USES it is the switch's business, strip_wide)
  if (strip_shape(a.L, true)) mem.get(&a.wt, mlp_strip_wt_floats(a.L.Dp, a.L.Op));
  if (strip_shape(cr.L, true)) mem.get(&cr.wt, mlp_strip_wt_floats(cr.L.Dp, cr.L.Op));
  if (a.wt && cr.wt && R % 64 == 0 && p->sw.strip_bits) {
    const size_t bw = mlp_strip_bits_words(R);   // per layer: 2 bw words for the actor's 2R rows, bw for the critic's
    mem.get(&a.bits1, 4 * bw); mem.get(&cr.bits1, 2 * bw);
    if (a.bits1 && cr.bits1) { a.bits2 = a.bits1 + 2 * bw; cr.bits2 = cr.bits1 + bw; }
  }
  if (a.wt && cr.wt) {
    mem.get(&p->stat_rows, NSTAT * R);
    mem.get(&p->wt_inf, WT_SLOTS * (mlp_strip_wt_floats(p->a.L.Dp, p->a.L.Op) + mlp_strip_wt_floats(p->c.L.Dp, p->c.L.Op)));
    mem.get(&p->wt_roll, mlp_strip_wt_floats(p->a.L.Dp, p->a.L.Op) + mlp_strip_wt_floats(p->c.L.Dp, p->c.L.Op));
  } else if (rollout_wide_supported(a.L)) {   // rows past the strips' capacity: the actor's copy for the in-wave step, nothing else reads one
    mem.get(&p->wt_roll, mlp_strip_wt_floats(p->a.L.Dp, p->a.L.Op));
  }
  const bool ok = !mem.failed() && learner_mirror(*p, c) && hipStreamCreateWithFlags(&p->side, hipStreamNonBlocking) == hipSuccess &&
                  hipEventCreateWithFlags(&p->ev_fork, hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&p->ev_join, hipEventDisableTiming) == hipSuccess &&
                  hipEventCreateWithFlags(&p->ev_head, hipEventDisableTiming) == hipSuccess;
  if (!ok) return lhw_fail(LHW_ERR_HIP, "PPO workspace allocation failed (max_rows=%d) or bad mirror table", c->max_rows);
  *out = p.release();
  return LHW_OK;
}

extern "C" int lhw_ppo_destroy(LhwPpo* p) { delete p; return LHW_OK; }   // (~LhwPpo: step graph, side stream, events; then the memory owner)

extern "C" int lhw_ppo_set_inference_dtype(LhwPpo* p, int fp16) {
  if (!p) return lhw_fail(LHW_ERR_ARG, "null ppo");
  p->infer_half = fp16 ? 1 : 0;
  return LHW_OK;
}

extern "C" int lhw_ppo_set_update_dtype(LhwPpo* p, int fp16) {
  if (!p) return lhw_fail(LHW_ERR_ARG, "null ppo");
  if (fp16 && !p->xb_h && p->sw.fp16_storage) {
    // fp16 HBM storage of the minibatch activations (round 6; LHW_FP16_STORAGE=0: float32 storage rounded per GEMM, as through round 5)
    // All or nothing: the handle's pointers are set once all nine blocks exist; a failure frees those obtained and leaves it as it was.
    HIPCHK(hipSetDevice(p->device));
    const size_t R = p->max_rows, H = p->H, ldxh = (p->a.L.Dp + 7) & ~7;
    _Float16** const dst[9] = {&p->xb_h, &p->a.h1_h, &p->a.h2_h, &p->a.dh2_h, &p->a.dh1_h, &p->c.h1_h, &p->c.h2_h, &p->c.dh2_h, &p->c.dh1_h};
    const size_t n[9] = {2 * R * ldxh, 2 * R * H, 2 * R * H, 2 * R * H, 2 * R * H, R * H, R * H, R * H, R * H};
    _Float16* got[9];
    const size_t mark = p->mem.mark();
    for (int i = 0; i < 9; i++) got[i] = p->mem.get<_Float16>(n[i]);
    if (p->mem.failed()) {
      p->mem.release_to(mark);
      return lhw_fail(LHW_ERR_HIP, "fp16 workspace allocation failed (max_rows=%d)", p->max_rows);
    }
    for (int i = 0; i < 9; i++) *dst[i] = got[i];
    p->ldxh = p->a.ldxh = p->c.ldxh = (int)ldxh;
    p->a.x_h = p->c.x_h = p->xb_h;
  }
  p->update_half = fp16 ? 1 : 0;
  return LHW_OK;
}

extern "C" int lhw_ppo_debug_set_strip_fused(LhwPpo* p, int32_t on) {
  if (!p) return lhw_fail(LHW_ERR_ARG, "null ppo");
  p->sw.strip_fused = on ? 1 : 0;
  return LHW_OK;
}

extern "C" int lhw_ppo_debug_set_strip_wide(LhwPpo* p, int32_t on) {
  if (!p) return lhw_fail(LHW_ERR_ARG, "null ppo");
  p->sw.strip_wide = on ? 1 : 0;
  p->roll_theta = nullptr;   // (an open bracket has the critic's weight copies of the other choice)
  return LHW_OK;
}

extern "C" int lhw_ppo_debug_set_strip_fp16(LhwPpo* p, int32_t on) {
  if (!p) return lhw_fail(LHW_ERR_ARG, "null ppo");
  if (on && !p->a.wh && strip_h_shape(p->a.L) && strip_h_shape(p->c.L)) {
    // the kernels' fp16 weight copies, one block: the update's pair, the rollout bracket's, WT_SLOTS pairs for forward calls outside a bracket
    HIPCHK(hipSetDevice(p->device));
    _Float16* wh = p->mem.get_lazy<_Float16>((size_t)(4 + 2 * WT_SLOTS) * MLP_STRIP_H_WH_HALVES, LhwDevMem::RAW);
    if (!wh) return lhw_fail(LHW_ERR_HIP, "fp16 strip weight copies: allocation failed");
    p->a.wh = wh; p->c.wh = wh + MLP_STRIP_H_WH_HALVES; p->wh_roll = wh + 2 * MLP_STRIP_H_WH_HALVES; p->wh_inf = wh + 4 * MLP_STRIP_H_WH_HALVES;
  }
  p->sw.strip_fp16 = on ? 1 : 0;
  p->roll_theta = nullptr;   // (an open bracket may not have the fp16 copies)
  return LHW_OK;
}

extern "C" int lhw_ppo_debug_last_grad_fused(const LhwPpo* p) { return p ? p->last_plan.train : LHW_ERR_ARG; }
// out13: UpdatePlan's eight fields for a minibatch of B rows (imitation != 0: with an imitation term armed), then InferPlan's five
extern "C" int lhw_ppo_debug_plan(const LhwPpo* p, int32_t B, int32_t imitation, int32_t* out13) {
  if (!p || !out13 || B <= 0 || B > p->max_rows) return lhw_fail(LHW_ERR_ARG, "bad argument (B = %d, capacity %d)", B, p ? p->max_rows : 0);
  const UpdatePlan u = update_plan(p, imitation != 0);
  const InferPlan i = infer_plan(p);
  memcpy(out13, &u, sizeof u); memcpy(out13 + sizeof u / sizeof(int32_t), &i, sizeof i);
  return LHW_OK;
}
extern "C" int64_t lhw_ppo_param_count(const LhwPpo* p) { return p ? (int64_t)p->n_params : LHW_ERR_ARG; }

// offsets (in floats) of each tensor inside the flat parameter vector:
// out[0..5] actor W1,b1,W2,b2,W3,b3 ; out[6] stds ; out[7..12] critic W1..b3 ; out[13] obs pad width Dp ; out[14] actor Op
extern "C" int lhw_ppo_layout(const LhwPpo* p, int64_t* out15) {
  if (!p || !out15) return lhw_fail(LHW_ERR_ARG, "null argument");
  const MlpLayout &a = p->a.L, &c = p->c.L;
  const size_t oa = p->off_actor, oc = p->off_critic;
  const size_t v[15] = {oa + a.w1, oa + a.b1, oa + a.w2, oa + a.b2, oa + a.w3, oa + a.b3, p->off_std,
                        oc + c.w1, oc + c.b1, oc + c.w2, oc + c.b2, oc + c.w3, oc + c.b3, (size_t)a.Dp, (size_t)a.Op};
  for (int i = 0; i < 15; i++) out15[i] = (int64_t)v[i];
  return LHW_OK;
}
extern "C" int lhw_ppo_normalize(LhwPpo* p, const float* obs, int64_t R, const float* obs_mean, const float* obs_std, float* xn, float* xm, void* stream) {
  return learner_normalize(p, obs, R, obs_mean, obs_std, xn, xm, stream);
}

// Rollout inference for N rows (N <= max_rows): normalise, actor + critic forward, sample.
//   act/logp/mu may be NULL to run the critic only; value may be NULL to run the actor only.
// ws_row: first row of the forward workspace to use (concurrent calls on different streams must use disjoint row ranges)
extern "C" int lhw_ppo_forward_at(LhwPpo* p, const float* theta, const float* obs, int64_t N, const float* obs_mean, const float* obs_std,
                                  uint64_t seed, uint32_t env_id_base, uint32_t counter, int deterministic, int64_t ws_row, float* mu,
                                  float* act, float* logp, float* value, void* stream) {
  if (!p || !theta || !obs || N <= 0 || ws_row < 0 || ws_row + N > p->max_rows)
    return lhw_fail(LHW_ERR_ARG, "bad argument (rows [%lld, %lld), capacity %d)", (long long)ws_row, (long long)(ws_row + N), p ? p->max_rows : 0);
  HIPCHK(hipSetDevice(p->device));
  hipStream_t s = (hipStream_t)stream;
  const size_t Dp = p->a.L.Dp, Op = p->a.L.Op, r0 = (size_t)ws_row;
  float *xb = p->xb + r0 * Dp, *ya = p->a.y + r0 * Op, *yc = p->c.y + r0 * 4;
  const RowSpan rows{r0, (int)N};
  const InferPlan ip = infer_plan(p);
  const float *tha = theta + p->off_actor, *thc = theta + p->off_critic;
  float *wta = nullptr, *wtc = nullptr;   // this call's weight copies for the strip kernel
  const bool wt_ready = p->roll_theta != nullptr && p->roll_theta == theta;   // inside a rollout bracket: made once by lhw_ppo_begin_rollout
  _Float16 *wha = nullptr, *whc = nullptr;   // ... for the fp16 forward strip
  if (ip.strips && !ip.half) {
    const size_t fa = mlp_strip_wt_floats(p->a.L.Dp, p->a.L.Op), fc = mlp_strip_wt_floats(p->c.L.Dp, p->c.L.Op);
    wta = wt_ready ? p->wt_roll : p->wt_inf + (size_t)(ws_row * WT_SLOTS / p->max_rows) * (fa + fc);
    wtc = wta + fa;
  } else if (ip.strips) {
    wha = wt_ready ? p->wh_roll : p->wh_inf + (size_t)(ws_row * WT_SLOTS / p->max_rows) * 2 * MLP_STRIP_H_WH_HALVES;
    whc = wha + MLP_STRIP_H_WH_HALVES;
  }
  // the rollout's policy step (actions + log-densities only) as ONE strip launch: observation normalisation on the way into the
  // slab, the three layers, the Gaussian head on the read-out -- instead of normalise / forward / sample launches
  // (the fused staging reads RAW observation rows of width obs_dim: without the normalisation vectors it would have to copy rows
  // of width Dp, which the caller's buffer does not have -- those calls take the three-launch path)
  if (ip.policy_step && act && logp && !mu && !value && obs_mean && obs_std) {
    const MlpLayout& La = p->a.L;
    if (!wt_ready) strip_prepare(La, tha, wta, s);
    const StripWeights w = strip_weights(La, wta, tha);
    MlpStripFwd a{w.w1t, w.b1, w.w2t, w.b2, w.w3t, w.b3, obs, p->D, La.Dp, La.O, La.Op, (int)N, nullptr, nullptr, ya};
    a.in_mean = obs_mean; a.in_std = obs_std; a.in_dim = p->D;
    a.stdv = theta + p->off_std; a.act = act; a.logp = logp;
    a.seed = seed; a.env_base = env_id_base; a.counter = counter; a.deterministic = deterministic;
    mlp_strip_forward(a, s);
    HIPCHK(hipGetLastError());
    return LHW_OK;
  }
  hipLaunchKernelGGL(normalize_kernel, dim3(((size_t)N * Dp + 255) / 256), dim3(256), 0, s, obs, p->D, p->a.L.Dp, (size_t)N, obs_mean, obs_std,
                     xb, (float*)nullptr, (const int*)nullptr, (const float*)nullptr);
  MlpPass m; m.half = ip.half;   // (h1 / h2 are not kept, no mask bits)
  if (act || mu) {
    if (wta && !wt_ready) strip_prepare(p->a.L, tha, wta, s);
    if (wha && !wt_ready) strip_h_prepare(p->a.L, tha, wha, s);
    m.wt = wta; m.wh = wha;
    mlp_forward(p->a, tha, rows, s, m);
    if (mu) HIPCHK(hipMemcpy2DAsync(mu, sizeof(float) * p->A, ya, sizeof(float) * p->a.L.Op, sizeof(float) * p->A, N, hipMemcpyDeviceToDevice, s));
    if (act) {
      if (!logp) return lhw_fail(LHW_ERR_ARG, "logp required with act");
      hipLaunchKernelGGL(sample_kernel, dim3((N + 7) / 8), dim3(256), 0, s, ya, p->a.L.Op, p->A, (int)N, theta + p->off_std, seed, env_id_base, counter, deterministic, act, logp);
    }
  }
  if (value) {
    if (wtc && !wt_ready) strip_prepare(p->c.L, thc, wtc, s);
    if (whc && !wt_ready) strip_h_prepare(p->c.L, thc, whc, s);
    m.wt = wtc; m.wh = whc;
    mlp_forward(p->c, thc, rows, s, m);
    HIPCHK(hipMemcpy2DAsync(value, sizeof(float), yc, sizeof(float) * 4, sizeof(float), N, hipMemcpyDeviceToDevice, s));
  }
  HIPCHK(hipGetLastError());
  return LHW_OK;
}

extern "C" int lhw_ppo_begin_rollout(LhwPpo* p, const float* theta, void* stream) {
  if (!p || !theta) return lhw_fail(LHW_ERR_ARG, "null argument");
  p->roll_theta = nullptr;
  const InferPlan ip = infer_plan(p);
  if (!ip.actor_copies) return LHW_OK;   // per-layer GEMM inference reads theta itself: nothing to prepare
  HIPCHK(hipSetDevice(p->device));
  hipStream_t s = (hipStream_t)stream;
  strip_prepare(p->a.L, theta + p->off_actor, p->wt_roll, s);   // (the critic's only where forward launches will read them)
  if (ip.critic_copies) strip_prepare(p->c.L, theta + p->off_critic, p->wt_roll + mlp_strip_wt_floats(p->a.L.Dp, p->a.L.Op), s);
  if (ip.critic_copies && p->sw.strip_fp16 && p->a.wh) {   // the fp16 forward strip's copies of both networks, whichever dtype is selected right now
    strip_h_prepare(p->a.L, theta + p->off_actor, p->wh_roll, s);
    strip_h_prepare(p->c.L, theta + p->off_critic, p->wh_roll + MLP_STRIP_H_WH_HALVES, s);
  }
  HIPCHK(hipGetLastError());
  p->roll_theta = theta;
  return LHW_OK;
}
extern "C" int lhw_ppo_end_rollout(LhwPpo* p) {
  if (!p) return lhw_fail(LHW_ERR_ARG, "null ppo");
  p->roll_theta = nullptr;
  return LHW_OK;
}

extern "C" int lhw_ppo_rollout_policy(LhwPpo* p, const float* theta, const float* obs_mean, const float* obs_std, uint64_t seed,
                                      uint32_t counter, int deterministic, LhwRolloutPolicy* out) {
  if (!p || !theta || !obs_mean || !obs_std || !out) return lhw_fail(LHW_ERR_ARG, "null argument");
  const MlpLayout& La = p->a.L;
  const InferPlan ip = infer_plan(p);
  if (p->roll_theta != theta || !ip.actor_copies)
    return lhw_fail(LHW_ERR_UNSUPPORTED, "lhw_ppo_rollout_policy: no rollout bracket open for this theta (lhw_ppo_begin_rollout)");
  const StripWeights w = strip_weights(La, p->wt_roll, theta + p->off_actor);
  out->w1t = w.w1t; out->b1 = w.b1; out->w2t = w.w2t; out->b2 = w.b2; out->w3t = w.w3t; out->b3 = w.b3;
  out->stdv = theta + p->off_std; out->obs_mean = obs_mean; out->obs_std = obs_std;
  out->obs_dim = p->D; out->obs_pad = La.Dp; out->act_dim = La.O; out->act_pad = La.Op; out->hidden = La.H;
  out->deterministic = deterministic; out->seed = seed; out->counter = counter;
  out->fp16_operands = ip.half ? 1 : 0;
  return LHW_OK;
}

extern "C" int lhw_ppo_forward(LhwPpo* p, const float* theta, const float* obs, int64_t N, const float* obs_mean, const float* obs_std, uint64_t seed,
                               uint32_t env_id_base, uint32_t counter, int deterministic, float* mu, float* act, float* logp, float* value, void* stream) {
  return lhw_ppo_forward_at(p, theta, obs, N, obs_mean, obs_std, seed, env_id_base, counter, deterministic, 0, mu, act, logp, value, stream);
}
// the spans of the actor's rows one pass covers for a minibatch of B rows in a workspace of R: the mirrored rows start at row R, so they
// follow the normal ones without a gap when B == R
struct RowSpans { RowSpan v[2]; int n; };
static RowSpans actor_spans(int mir, int B, int R) {
  if (mir && B == R) return {{{0, 2 * B}, {0, 0}}, 1};
  return {{{0, B}, {(size_t)R, B}}, mir ? 2 : 1};
}
// gather_kernel's argument for a minibatch, for its launch and for the patch of its captured launch (lhw_ppo_step)
static GatherArgs gather_args(const LhwPpo* p, const float* xn, const float* xm, const float* act, const float* old_logp, const float* adv, const float* ret, const int32_t* idx, int32_t B) {
  return GatherArgs{idx, B, p->max_rows, p->a.L.Dp, p->A, xn, p->use_mirror ? xm : nullptr, act, old_logp, adv, ret, p->xb, p->mb_act, p->mb_logp, p->mb_adv, p->mb_ret};
}

// Arms the imitation term for the next lhw_ppo_grad call: target / mask are device arrays [B][act_dim] in minibatch row
// order (row r belongs to idx[r]); n_selected = number of set mask entries (the mean's denominator).
extern "C" int lhw_ppo_set_imitation(LhwPpo* p, const float* target, const uint8_t* mask, float coeff, int64_t n_selected) {
  if (!p) return lhw_fail(LHW_ERR_ARG, "null ppo");
  if (!target || !mask || n_selected <= 0) { p->imit_target = nullptr; p->imit_mask = nullptr; return LHW_OK; }
  p->imit_target = target; p->imit_mask = mask; p->imit_coeff = coeff; p->imit_inv_count = 1.f / (float)n_selected;
  return LHW_OK;
}

// One minibatch: gather rows idx[0..B) from the iteration's buffers, forward (policy on obs and on mirrored
// obs, critic), losses, backward.  Gradients are ACCUMULATED into grad (flat, same layout as theta);
// stats_dev[0..4] += actor_loss, critic_loss, mirror_loss, approx_kl, clip_fraction of this minibatch.
extern "C" int lhw_ppo_grad(LhwPpo* p, const float* theta, float* grad, const float* xn, const float* xm, const float* act, const float* old_logp,
                            const float* adv, const float* ret, const int32_t* idx, int32_t B, float* stats_dev, void* stream) {
  if (!p || !theta || !grad || !xn || !act || !old_logp || !adv || !ret || !idx || !stats_dev) return lhw_fail(LHW_ERR_ARG, "null argument");
  if (B <= 0 || B > p->max_rows) return lhw_fail(LHW_ERR_ARG, "minibatch %d exceeds workspace capacity %d", B, p->max_rows);
  const int mir = p->use_mirror && xm != nullptr;
  HIPCHK(hipSetDevice(p->device));
  hipStream_t s = (hipStream_t)stream;
  const MlpNet &na = p->a, &nc = p->c;
  const MlpLayout &La = na.L, &Lc = nc.L;
  const int R = p->max_rows, Dp = La.Dp, Op = La.Op;
  const float *th_a = theta + p->off_actor, *th_c = theta + p->off_critic;
  const UpdatePlan u = p->last_plan = update_plan(p, p->imit_target != nullptr);
  const StreamPair sp{s, u.streams == 2 ? p->side : s, p->ev_fork, p->ev_join};
  hipStream_t sc = sp.sc;   // the critic's chain
  const RowSpans spans = actor_spans(mir, B, R); const RowSpan rows_c{0, B};
  // ---- prologue
  // the [in][out] weight copies of the forward strips are made on the side stream while the minibatch is gathered (round 6: the two
  // 9 us transposes were the first links of the step's chain)
  const int strips = u.train ? 3 : u.fwd_strip;   // the networks whose copies a launch of this step reads (fp16 operands: the fp16 copies)
  if (strips) sp.fork();
  if (strips & 1) { if (u.half) strip_h_prepare(La, th_a, na.wh, sc); else strip_prepare(La, th_a, na.wt, sc); }
  if (strips & 2) { if (u.half) strip_h_prepare(Lc, th_c, nc.wh, sc); else strip_prepare(Lc, th_c, nc.wt, sc); }
  hipLaunchKernelGGL(gather_kernel, dim3(((size_t)B * Dp + 255) / 256), dim3(256), 0, s, gather_args(p, xn, xm, act, old_logp, adv, ret, idx, B));
  if (strips) sp.join();
  // --fp16 update with fp16 storage: fp16 copies of the gathered rows; every activation the GEMMs exchange stays fp16 in HBM
  for (int i = 0; u.hstore && i < spans.n; i++) {
    const RowSpan r = spans.v[i];
    const size_t nn = (size_t)r.rows * p->ldxh;
    hipLaunchKernelGGL(rows_to_half_kernel, dim3((nn + 255) / 256), dim3(256), 0, s, p->xb + r.first * Dp, Dp, Dp, (size_t)r.rows, p->xb_h + r.first * p->ldxh, p->ldxh);
  }
  const BwdParts Pa = bwd_parts_carve(La, R, 2, p->bwd_part);
  const BwdParts Pc = bwd_parts_carve(Lc, R, 1, p->bwd_part + bwd_parts_floats(La, R, 2));
  BwdSlices za, zc;
  // Train strips: per network ONE launch runs the forward layers, the loss head and the backward layers (mlp_train_strip_kernel) -- no join
  // between the passes, no loss launch, no mask bits; the weight-gradient kernels follow as on the other path.  With mirroring a slab pairs
  // 32 rows with their twins, whatever B (a ragged last slab has dead rows in both tiles).  Where the plan has none: forward strip (or GEMMs),
  // ppo_loss_kernel, backward.
  const bool fused = u.train != 0;
  MlpPass ma;
  ma.half = u.half; ma.hstore = u.hstore; ma.keep = true; ma.bits = u.bits; ma.have_dh = fused;
  MlpPass mc = ma;
  ma.wt = !u.half && (u.fwd_strip & 1) ? na.wt : nullptr; ma.wh = u.half && (u.fwd_strip & 1) ? na.wh : nullptr; ma.bwd_strip = u.bwd_strip & 1;
  mc.wt = !u.half && (u.fwd_strip & 2) ? nc.wt : nullptr; mc.wh = u.half && (u.fwd_strip & 2) ? nc.wh : nullptr; mc.bwd_strip = u.bwd_strip & 2;
  const int nblk = (B + 255) / 256;
  // fp16 update: the back-propagated gradients are rounded to fp16 per GEMM, and d loss / d output carries 1 / B -- at B = 32768
  // most of it would fall into the fp16 subnormal range.  Loss scaling by a power of two (exact in float32): the read-out
  // gradients are multiplied by 2^ceil(log2 B) by the loss kernel and the weight-gradient totals divided by it in the final ordered reduction.
  const float lscale = u.half ? exp2f(ceilf(log2f((float)B))) : 1.f;
  // ---- forward and loss; on the fused path the critic's backward too (its launches sit between the two train strips' on the side stream)
  if (fused) {
    const LhwPpoHead head{B, p->A, Op, p->mb_act, p->mb_logp, p->mb_adv, p->mb_ret, theta + p->off_std, p->clip, p->mirror_coeff, mir, p->d_act_src,
                          p->d_act_sign, p->learn_std ? p->dstd : (float*)nullptr, nullptr, nullptr, 0.f, 0.f, 1.f};
    auto train = [&](const MlpNet& n, const float* th, int twin0, int critic, hipStream_t st) {
      const MlpLayout& L = n.L;
      const StripWeights w = strip_weights(L, n.wt, th);
      MlpStripTrain t{MlpStripFwd{w.w1t, w.b1, w.w2t, w.b2, w.w3t, w.b3, p->xb, Dp, L.Dp, L.O, L.Op, B, n.h1, n.h2, nullptr},
                      th + L.w2, th + L.w3, n.dy, n.dh2, n.dh1, twin0, critic, head, p->stat_rows, R};
      mlp_train_strip(t, st);
    };
    sp.fork();
    train(nc, th_c, 0, 1, sc);
    mlp_backward(nc, th_c, rows_c, Pc, zc, sc, mc);
    train(na, th_a, mir ? R : 0, 0, s);
    // (the step's loss statistics -- logging only -- are summed at the tail of the side stream, off both chains, once the actor's rows are there)
    if (sc != s) { (void)hipEventRecord(p->ev_head, s); (void)hipStreamWaitEvent(sc, p->ev_head, 0); }
    hipLaunchKernelGGL(ppo_stats_rows_kernel, dim3(nblk), dim3(256), 0, sc, B, p->A, p->stat_rows, R, p->imit_inv_count, p->stats_part);
    hipLaunchKernelGGL(reduce_rows_kernel, dim3(1), dim3(64), 0, sc, p->stats_part, nblk, NSTAT, stats_dev);
  } else {
    sp.fork();
    mlp_forward(nc, th_c, rows_c, sc, mc);
    for (int i = 0; i < spans.n; i++) mlp_forward(na, th_a, spans.v[i], s, ma);
    sp.join();
    hipLaunchKernelGGL(ppo_loss_kernel, dim3(nblk), dim3(256), 0, s, B, R, p->A, Op, na.y, nc.y, p->mb_act, p->mb_logp,
                       p->mb_adv, p->mb_ret, theta + p->off_std, p->clip, p->mirror_coeff, mir, p->d_act_src, p->d_act_sign, na.dy,
                       nc.dy, p->learn_std ? p->dstd : (float*)nullptr, p->stats_part, p->imit_target, p->imit_mask, p->imit_coeff,
                       p->imit_inv_count, 0, lscale);
    p->imit_target = nullptr; p->imit_mask = nullptr;   // armed for one call only
  }
  // ---- epilogue: the gradient of the stds, the weight gradients, their ordered reduction
  if (p->learn_std) {
    colsum_det(p->dstd, B, Op, p->A, grad + p->off_std, p->part, s);
    hipLaunchKernelGGL(entropy_grad_kernel, dim3(1), dim3(64), 0, s, theta + p->off_std, p->A, p->ent_coeff, grad + p->off_std);
  }
  if (!fused) {
    sp.fork();
    // (the step's loss statistics -- logging only -- are summed at the head of the side stream, off the actor's chain)
    hipLaunchKernelGGL(reduce_rows_kernel, dim3(1), dim3(64), 0, sc, p->stats_part, nblk, NSTAT, stats_dev);
    mlp_backward(nc, th_c, rows_c, Pc, zc, sc, mc);
  }
  for (int i = 0; i < spans.n; i++) mlp_backward(na, th_a, spans.v[i], Pa, za, s, ma);
  sp.join();
  SegList S; S.n = 0; S.scale = 1.f / lscale;
  mlp_backward_segments(S, La, grad + p->off_actor, Pa, za);
  mlp_backward_segments(S, Lc, grad + p->off_critic, Pc, zc);
  launch_reduce_segments(S, s);
  HIPCHK(hipGetLastError());
  return LHW_OK;
}

extern "C" int lhw_ppo_apply(LhwPpo* p, float* theta, float* grad, float* adam_m, float* adam_v, int64_t step, float grad_scale, void* stream) {
  if (p) p->roll_theta = nullptr;   // theta changes: the weight copies of an open rollout bracket are stale
  return learner_apply(p, theta, grad, adam_m, adam_v, step, grad_scale, stream);
}
extern "C" int lhw_ppo_debug_grad_sqnorms(LhwPpo* p, float* out2_host) { return learner_grad_sqnorms(p, out2_host); }
// One optimiser step as ONE graph launch.  lhw_ppo_grad + lhw_ppo_apply are some forty launches on two streams, a dozen of them small (gather,
// loss, ordered reductions, transposes, clip, Adam: 5-20 us of work each behind a launch gap of the same order); captured once per StepKey as a
// hipGraph they replay with one host call and the runtime's graph scheduling between the nodes.  Same kernels, same order, same arithmetic: bitwise
// the weights of the two-call path (tests/test_iteration_gpu.py, tests/test_optimizer_gpu.py).  What changes from step to step is patched into the
// executable graph: the minibatch's index pointer (in gather_kernel's argument) and Adam's bias corrections (in adam2_kernel's).  A different
// grad_scale recaptures: it is also an argument of sumsq2_kernel, whose node is not patched.  Single process only -- with data parallelism the gradient
// all-reduce sits between the two halves (the Python layer then keeps lhw_ppo_grad / all-reduce / lhw_ppo_apply).  LHW_PPO_GRAPH=0: the two calls, eagerly.
// replaces the argument of a captured launch of a kernel whose one parameter is a by-value struct
static int patch_kernel_arg(hipGraphExec_t exec, hipGraphNode_t node, void* arg) {
  void* args[1] = {arg};
  hipKernelNodeParams kp;
  HIPCHK(hipGraphKernelNodeGetParams(node, &kp));
  kp.kernelParams = args; kp.extra = nullptr;
  HIPCHK(hipGraphExecKernelNodeSetParams(exec, node, &kp));
  return LHW_OK;
}
extern "C" int lhw_ppo_step(LhwPpo* p, float* theta, float* grad, float* adam_m, float* adam_v, const float* xn, const float* xm, const float* act,
                            const float* old_logp, const float* adv, const float* ret, const int32_t* idx, int32_t B, float* stats_dev,
                            int64_t step, float grad_scale, void* stream) {
  if (!p || !theta || !grad || !adam_m || !adam_v || !idx || step <= 0) return lhw_fail(LHW_ERR_ARG, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  // (an armed imitation term is a one-shot argument of the next lhw_ppo_grad: not captured; the legacy default stream cannot be captured)
  if (!p->sw.graph || p->imit_target != nullptr || s == nullptr) {
    const int rc = lhw_ppo_grad(p, theta, grad, xn, xm, act, old_logp, adv, ret, idx, B, stats_dev, stream);
    return rc ? rc : lhw_ppo_apply(p, theta, grad, adam_m, adam_v, step, grad_scale, stream);
  }
  HIPCHK(hipSetDevice(p->device));
  StepKey key{{theta, grad, adam_m, adam_v, xn, xm, act, old_logp, adv, ret, stats_dev, stream}, B, 0, update_plan(p, false)};
  memcpy(&key.gs, &grad_scale, sizeof key.gs);
  if (!p->step_exec || !(p->step_key == key)) {
    if (p->step_exec) { (void)hipGraphExecDestroy(p->step_exec); p->step_exec = nullptr; }
    if (p->step_graph) { (void)hipGraphDestroy(p->step_graph); p->step_graph = nullptr; }
    p->node_gather = p->node_adam = nullptr;
    HIPCHK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    int rc = lhw_ppo_grad(p, theta, grad, xn, xm, act, old_logp, adv, ret, idx, B, stats_dev, stream);
    if (!rc) rc = lhw_ppo_apply(p, theta, grad, adam_m, adam_v, step, grad_scale, stream);
    hipGraph_t g = nullptr;
    const hipError_t ec = hipStreamEndCapture(s, &g);
    if (rc) { if (g) (void)hipGraphDestroy(g); return rc; }
    if (ec != hipSuccess || !g) return lhw_fail(LHW_ERR_HIP, "lhw_ppo_step: stream capture failed: %s", hipGetErrorString(ec));
    p->step_graph = g;
    size_t nn = 0;
    HIPCHK(hipGraphGetNodes(g, nullptr, &nn));
    std::vector<hipGraphNode_t> nodes(nn);
    HIPCHK(hipGraphGetNodes(g, nodes.data(), &nn));
    for (hipGraphNode_t nd : nodes) {
      hipGraphNodeType ty;
      if (hipGraphNodeGetType(nd, &ty) != hipSuccess || ty != hipGraphNodeTypeKernel) continue;
      hipKernelNodeParams kp;
      if (hipGraphKernelNodeGetParams(nd, &kp) != hipSuccess) continue;
      if (kp.func == (void*)gather_kernel) p->node_gather = nd;
      else if (kp.func == (void*)adam2_kernel) p->node_adam = nd;
    }
    if (!p->node_gather || !p->node_adam) return lhw_fail(LHW_ERR_HIP, "lhw_ppo_step: gather / Adam nodes not found in the captured graph (%zu nodes)", nn);
    HIPCHK(hipGraphInstantiate(&p->step_exec, g, nullptr, nullptr, 0));
    p->step_key = key;
  }
  // patch the two nodes: each kernel's one argument, built by the function that builds it for the launch
  GatherArgs ga = gather_args(p, xn, xm, act, old_logp, adv, ret, idx, B);
  AdamArgs aa = learner_adam_args(*p, theta, grad, adam_m, adam_v, step, grad_scale);
  if (const int rc = patch_kernel_arg(p->step_exec, p->node_gather, &ga)) return rc;
  if (const int rc = patch_kernel_arg(p->step_exec, p->node_adam, &aa)) return rc;
  p->roll_theta = nullptr;
  HIPCHK(hipGraphLaunch(p->step_exec, s));
  return LHW_OK;
}
