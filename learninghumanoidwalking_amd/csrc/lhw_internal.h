// Internal (non-ABI) interfaces between the translation units of liblhw.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/lhw.h"
#include "lhw_ppo_head.h"

int lhw_fail(int code, const char* fmt, ...);
#define HIPCHK(x)                                                                                   \
  do {                                                                                              \
    hipError_t e_ = (x);                                                                            \
    if (e_ != hipSuccess) return lhw_fail(LHW_ERR_HIP, "%s failed: %s", #x, hipGetErrorString(e_)); \
  } while (0)
static inline int pad4(int x) { return (x + 3) & ~3; }

// POISON MODE (debug): nothing on the GPU zero-fills LDS, and what a workgroup finds there is whatever the previous occupant
// of the CU left -- another kernel, another process.  LHW_LDS_POISON(obj), placed right behind a __shared__ declaration,
// fills the object with 0xFF bytes (NaN as float / double, -1 as int) in the SIMT emulator of tests/emu (always) and in a
// -DLHW_POISON build of the GPU library (scripts/build_variant.sh), so that a read of a never-written word shows up as a NaN
// instead of depending on the CU's history.  A no-op in the product build.
#if defined(__HIP_EMU__)
#define LHW_LDS_POISON(obj) emu::poison_shared((void*)&(obj), sizeof(obj))
#elif defined(LHW_POISON)
#define LHW_LDS_POISON(obj)                                                                                            \
  do {                                                                                                                 \
    unsigned* w_ = reinterpret_cast<unsigned*>(&(obj));                                                                \
    for (unsigned i_ = threadIdx.x; i_ < sizeof(obj) / 4; i_ += blockDim.x) w_[i_] = 0xFFFFFFFFu;                      \
    __syncthreads();                                                                                                   \
  } while (0)
#else
#define LHW_LDS_POISON(obj) ((void)0)
#endif
// device allocations of the library: 0xFF-filled when LHW_POISON=1 is set in the environment (hipMalloc does not zero either)
hipError_t lhw_malloc(void** p, size_t n);
template <class T> static inline hipError_t lhw_malloc(T** p, size_t n) { return lhw_malloc((void**)p, n); }

// The device memory of one handle (LhwEnv, HumanoidEnv, LhwPpo, LhwRnn).  Every block is recorded the moment lhw_malloc returns it, so
// no failure path can drop one, and the destructor frees them all on the handle's device.  A failed allocation or fill returns NULL and
// latches failed(): the calls after it return NULL without trying, so a run of allocations needs ONE check at its end.
// Lazy allocations on a live handle are transactions: m = mark() first, release_to(m) on failure -- the blocks obtained since are
// freed, the latch is cleared, and the handle owns what it owned before.
class LhwDevMem {
 public:
  int device = 0;
  LhwDevMem() = default;
  LhwDevMem(const LhwDevMem&) = delete;
  LhwDevMem& operator=(const LhwDevMem&) = delete;
  ~LhwDevMem() { release_to(0); }
  enum Fill { RAW, ZERO };
  // max(n, 1) elements of T, zero-filled unless RAW
  template <class T> T* get(size_t n, Fill fill = ZERO) {
    const size_t bytes = sizeof(T) * (n ? n : 1);
    void* d = nullptr;
    if (failed_ || lhw_malloc(&d, bytes) != hipSuccess || !d) { failed_ = true; return nullptr; }
    blocks_.push_back(d);
    if (fill == ZERO && hipMemset(d, 0, bytes) != hipSuccess) { failed_ = true; return nullptr; }
    return (T*)d;
  }
  template <class T> void get(T** out, size_t n, Fill fill = ZERO) { *out = get<T>(n, fill); }
  // a block of max(n, 1) elements holding a copy of host[0 .. n)
  template <class T> T* put(const T* host, size_t n) {
    T* d = get<T>(n, RAW);
    if (d && n && hipMemcpy(d, host, sizeof(T) * n, hipMemcpyHostToDevice) != hipSuccess) { failed_ = true; return nullptr; }
    return d;
  }
  // one block as a transaction of its own (diagnostic and export buffers enabled on a live handle)
  template <class T> T* get_lazy(size_t n, Fill fill = ZERO) {
    const size_t m = mark();
    T* d = get<T>(n, fill);
    if (!d) release_to(m);
    return d;
  }
  bool failed() const { return failed_; }
  size_t mark() const { return blocks_.size(); }
  void release_to(size_t mark) {
    if (blocks_.size() > mark) (void)hipSetDevice(device);
    while (blocks_.size() > mark) { (void)hipFree(blocks_.back()); blocks_.pop_back(); }
    failed_ = false;
  }

 private:
  std::vector<void*> blocks_;
  bool failed_ = false;
};

// The block of the per-term episode statistics (lhw_env_enable_term_stats), two arrays in one allocation: [N][LHW_MAX_REWARD_TERMS] sums
// of each env's RUNNING episode, then [N][LHW_TS_FIN_STRIDE] per env the sums over its FINISHED episodes since the last pop [k] and how
// many of those terminated / were truncated.  Only the env's own lane writes its rows, and lhw_env_pop_term_stats adds the finished rows
// up on the host in env order and clears that array: no atomics, and the popped sums do not depend on which wavefront finished first
// (two runs of the same rollout give the same bits).
enum { LHW_TS_TERMINATED = LHW_MAX_REWARD_TERMS, LHW_TS_TRUNCATED = LHW_MAX_REWARD_TERMS + 1, LHW_TS_FIN_STRIDE = LHW_MAX_REWARD_TERMS + 2 };

struct HumanoidEnv;
int humanoid_create(HumanoidEnv** out, const std::vector<int32_t>& mi, const std::vector<double>& md, const LhwEnvConfig* cfg,
                    int* obs_dim, int* act_dim, int* n_terms);
void humanoid_destroy(HumanoidEnv* h);
void humanoid_reset(HumanoidEnv* h, const uint8_t* mask, float* obs, hipStream_t s);
void humanoid_step(HumanoidEnv* h, const float* act, float* obs, float* term_obs, float* rew, uint8_t* done, float* rew_terms,
                   hipStream_t s);
int humanoid_step_range(HumanoidEnv* h, int first, int count, const float* act, float* obs, float* term_obs, float* rew, uint8_t* done,
                        float* rew_terms, hipStream_t s);
int humanoid_last_rollout_queued(const HumanoidEnv* h);
// One resident rollout, whatever the policy kind, as the API layer hands it to lhw_humanoid_rollout.hip.  Policy kinds: the feed-forward actor,
// the LSTM actor, the feed-forward actor on an observation history (rows of history_len x the env's base width).
enum { POLICY_MLP = 0, POLICY_LSTM = 1, POLICY_HIST = 2 };
struct HumanoidRollout {
  int first, count, T;
  float *obs, *act, *logp, *term_obs, *rew;
  uint8_t* done;
  float* rew_terms;                             // nullable
  double *tin_all, *stin_all;                   // nullable: the task-input record(s) of every control step
  int kind = POLICY_MLP;
  const LhwRolloutPolicy* mlp = nullptr;        // the view of POLICY_MLP and POLICY_HIST
  const LhwRolloutLstmPolicy* lstm = nullptr;   // ... of POLICY_LSTM
  const uint8_t* reset0 = nullptr;              // POLICY_LSTM
  int history_len = 1;                          // > 1: POLICY_HIST
};
// -1 bad range, -2 / -3 unsupported, -4 HIP error, -5 a diagnostic clock is armed and the rollout's kernel family has no clocks,
// -6 the actuator randomisation is armed and the rollout's policy kind has no kernels that carry it
int humanoid_rollout(HumanoidEnv* h, const HumanoidRollout& rq, hipStream_t s);
// width of a task's base observation (the kernels' TASK_* ids are the ABI's LHW_TASK_* values: lhw_humanoid.hip)
constexpr int humanoid_base_obs_dim(int task) {
  return task == LHW_TASK_JVRC_WALK ? 37 : (task == LHW_TASK_JVRC_STEP ? 39 : (task == LHW_TASK_H1_WALK ? 43 : 35));
}
void humanoid_get_state(HumanoidEnv* h, double* qpos, double* qvel, hipStream_t s);
void humanoid_set_state(HumanoidEnv* h, const double* qpos, const double* qvel, hipStream_t s);
double* humanoid_ep_stats(HumanoidEnv* h);
double* humanoid_term_stats(HumanoidEnv* h);                   // the term-statistics block the kernels write (NULL = off)
int humanoid_set_term_stats(HumanoidEnv* h, double* block);    // hands it to the kernels (NULL stops them); -1 HIP error, -2 a diagnostic clock is armed
// task shaping (lhw_env_set_task_shaping): weights [LHW_MAX_REWARD_TERMS] / limits [LHW_TERM_LIMIT_COUNT] of the host mirror; the setter
// takes validated values (either half may be NULL), uploads the parameters and returns -1 on a HIP error
void humanoid_get_task_shaping(const HumanoidEnv* h, double* weights, double* limits);
int humanoid_set_task_shaping(HumanoidEnv* h, const double* weights, int n_weights, const double* limits);
void humanoid_set_iteration(HumanoidEnv* h, int64_t it);
int humanoid_occupancy();
// The diagnostic clocks (phase clock: humanoid_profile, wave clock: humanoid_wave_cycles).  Once one is armed, control steps run the kernels
// that carry the clocks (humanoid_diag_kernel, humanoid_rollout_diag_kernel); the term statistics have kernels of their own, without clocks,
// so the two exclude each other: arming returns -2 while the statistics are on, -3 while the actuator randomisation is armed, -1 on a HIP error
bool humanoid_diag_armed(const HumanoidEnv* h);
// Actuator randomisation (lhw_env_set_actuator_randomization).  While pdrand_k > 0 or sim_bemf is set, control steps run the kernels that carry
// it (humanoid_act_kernel / humanoid_act_stats_kernel, humanoid_rollout_act_kernel / humanoid_rollout_act_stats_kernel); the clocks' kernels and
// the LSTM / history rollout kernels do not, so arming refuses while a clock is armed (-2) and those rollouts are declined while it is armed.
// The setter takes validated values, zeroes every env's tau_d when it turns sim_bemf off, uploads the parameters; -1 on a HIP error
bool humanoid_act_armed(const HumanoidEnv* h);
void humanoid_get_actuator_rand(const HumanoidEnv* h, LhwActuatorRand* out);
int humanoid_set_actuator_rand(HumanoidEnv* h, const LhwActuatorRand* a);
int humanoid_bemf_damping(HumanoidEnv* h, double* out /* [N][nu] host */);
// Task commands (lhw_env_set_task_commands / lhw_env_pin_commands).  The setters take validated values and upload the parameters; -1 on a
// HIP error.  The pin array -- device rows {mode or -1, mode_ref[3]} and a host mirror the getter answers from -- is created, every row
// free, by the first pin call; freeing every env afterwards keeps it (the kernels find no mode in any row)
void humanoid_get_task_commands(const HumanoidEnv* h, LhwTaskCommands* out);
int humanoid_set_task_commands(HumanoidEnv* h, const LhwTaskCommands* c);
int humanoid_pin_commands(HumanoidEnv* h, int first, int count, const int32_t* mode, const double* ref /* [count][3] */);
void humanoid_get_pinned_commands(const HumanoidEnv* h, int32_t* mode /* [N] */, double* ref /* [N][3] */);
// Pinned footstep plans of the stepping task (lhw_env_pin_step_plans): the same contract as the pin array above -- validated values in,
// created with every row free by the first call, kept when every env is freed, -1 on a HIP error; the host mirror holds the rows as the
// getter reports them (a free row: mode -1 and zeros; steps beyond nseq: zeros).  humanoid_step_nplans: rows of the env's plan table
int humanoid_step_nplans(const HumanoidEnv* h);
int humanoid_pin_step_plans(HumanoidEnv* h, int first, int count, const LhwStepPin* pins);
void humanoid_get_pinned_step_plans(const HumanoidEnv* h, LhwStepPin* out /* [N] */);
int humanoid_wave_cycles(HumanoidEnv* h, long long* out);
int humanoid_profile(HumanoidEnv* h, int enable, long long* out16);
// step_record: the stepping task's second record (LhwStepTaskInput) instead of LhwTaskInput; -1 HIP error, -2 not enabled
int humanoid_task_inputs(HumanoidEnv* h, bool step_record, int enable /* -1: leave */, double* out_host, double** out_dev);
int humanoid_actuator_state(HumanoidEnv* h, double* pos, double* vel, double* tq);
int humanoid_step_record(HumanoidEnv* h, double* seq, double* floor_z, int32_t* istate);

// LDS-resident strip kernels of the 3-layer MLPs (lhw_mlp_strip.hip); hidden width 256 only, callers fall back to the per-layer
// GEMMs otherwise.  Two sets of instantiations by padded input width Dp, picked by the launchers: narrow (Dp <= 64: mlp_strip_supported) and
// wide (64 < Dp <= LHW_MLP_STRIP_MAX_IN_PAD: mlp_strip_wide_supported; the read-out is then the GEMM path's single chain)
struct MlpStripFwd {
  const float *w1t, *b1, *w2t, *b2, *w3t, *b3;   // TRANSPOSED weights ([in][out]: W1^T [Dp][256], W2^T [256][256], W3^T [256][Op]) from mlp_strip_prepare
  const float* x; int ldx;                   // [R][ldx] inputs (Dp used columns)
  int Dp, O, Op, R;
  float *h1, *h2, *y;                        // [R][256], [R][256], [R][Op]; h1 / h2 may be NULL (inference: not written to HBM)
  // optional fusions for rollout inference (all NULL / 0 otherwise):
  const float *in_mean = nullptr, *in_std = nullptr; int in_dim = 0;   // x holds RAW observations [R][ldx = in_dim]: the slab is staged
                                                                      // as (x - mean) / std for columns < in_dim, zero up to Dp
  const float* stdv = nullptr;               // Gaussian head on the read-out (lhw_policy.h): act [R][O] = sample(y, stdv), logp [R]
  float *act = nullptr, *logp = nullptr;
  unsigned long long seed = 0; unsigned env_base = 0, counter = 0; int deterministic = 0;
  // optional (the update, 64-row slabs only): the ReLU masks of h1 / h2 as bits, mlp_strip_bits_words(R) words each, for the backward launch
  // over the SAME rows (same first row, same R): see store_act_t
  unsigned *bits1 = nullptr, *bits2 = nullptr;
};
struct MlpStripBwd {
  const float *w2, *w3, *dy, *h1, *h2;       // torch Linear layout [out][in]: W2 [256][256], W3 [Op][256]; dy [R][Op]
  int O, Op, R;
  float *dh2, *dh1;                          // [R][256] each
  const unsigned *bits1 = nullptr, *bits2 = nullptr;   // the forward launch's mask bits: h1 / h2 are then not read
};
// One network's whole pass over a minibatch in ONE launch (mlp_train_strip_kernel): forward layers, the PPO head on the read-out while it
// is still in LDS, backward layers -- a 64-row slab never leaves its workgroup, and y, dy's read-back and the ReLU mask bits never
// touch HBM.  f: the forward launch's arguments (R = live rows B; h1 / h2 are written, y only if not NULL; no inference fusions).
struct MlpStripTrain {
  MlpStripFwd f;
  const float *w2, *w3;                      // torch layout, as MlpStripBwd
  float *dy, *dh2, *dh1;                     // dy [.][Op] is still written once: the weight-gradient kernels read it
  int twin0;                                 // 0: slabs of 64 consecutive rows.  > 0 (actor with mirroring): row tile 0 = rows [r0, r0 + 32), row
                                             // tile 1 = their mirrored twins [twin0 + r0, twin0 + r0 + 32): a row and its twin meet in one workgroup
  int critic;                                // 0: actor head (lhw_ppo_actor_row), 1: critic head (O = 1)
  LhwPpoHead head;
  float* stat_rows; int stat_ld;             // [NSTAT][stat_ld]: every live row's terms of the loss scalars (the actor's launch writes all but
};                                           // term 1, the critic's term 1)
bool mlp_train_strip_supported(int H, int Dp, int O, int Op, int critic);            // the narrow train strip takes this shape
bool mlp_train_strip_wide_supported(int H, int Dp, int O, int Op, int critic);       // the wide one does
void mlp_train_strip(const MlpStripTrain& t, hipStream_t s);
size_t mlp_strip_bits_words(size_t rows);    // words per layer of the mask bits of a launch over `rows` rows (64-row slabs)
bool mlp_strip_supported(int H, int Dp, int O, int Op);        // the narrow forward / backward strips take this shape
bool mlp_strip_wide_supported(int H, int Dp, int O, int Op);   // the wide forward strip does (the backward strip has no input-width bound)
size_t mlp_strip_wt_floats(int Dp, int Op);
// WT [cols][ldt] <- W [rows][ld] for up to three matrices in one launch (mlp_strip_prepare's kernel; rows == 0: no matrix)
struct LhwTransposeJob { const float* W; float* WT; int rows, cols, ld, ldt; };
void lhw_transpose3(const LhwTransposeJob (&jobs)[3], hipStream_t s);
void mlp_strip_prepare(const float* w1, const float* w2, const float* w3, int Dp, int O, int Op, float* wt, hipStream_t s);
void mlp_strip_forward(const MlpStripFwd& a, hipStream_t s, int shape = 0);   // shape: 0 by row count, 1 small (32-row slabs), 2 big (64-row)
void mlp_strip_backward(const MlpStripBwd& a, hipStream_t s);

// Whole-sequence LSTM strip kernels of the recurrent update (lhw_mlp_strip.hip: lstm_seq_fwd_strip_kernel / lstm_seq_bwd_strip_kernel): the
// time loops of lhw_rnn_grad's forward pass and BPTT for one network (two stacked cells) as one launch each.  A workgroup owns 32 rows b of
// the [T][Bt] minibatch for all T steps.  Buffers are lhw_rnn.hip's SeqWs (rows r = t * Bt + b).
struct LstmSeqStrip {
  const float *w1t, *w2t;                    // forward: [in][out] copies from lstm_seq_strip_prepare, [Dp + H][4H] and [2H][4H]
  const float *w1, *w2;                      // backward: theta's own [4H][Dp + H] = [W_ih1 | W_hh1] and [4H][2H] = [W_ih2 | W_hh2]
  const float *bi1, *bh1, *bi2, *bh2;        // [4H] each
  float *xh1, *xh2, *g1, *g2, *c1, *c2, *h2; // [R][Dp + H] (x columns: input), [R][2H], [R][4H] x 2, [R][H] x 3
  const float* dh2;                          // backward: d loss / d h2 [R][H]
  const unsigned char* reset;                // [T][Bt]: an episode starts at step t of row b
  int T, Bt, H, Dp;
};
bool lstm_seq_strip_supported(int H, int Dp);   // LHW_LSTM_SEQ_* bounds of include/lhw.h
size_t lstm_seq_strip_wt_floats(int H, int Dp);
void lstm_seq_strip_prepare(const float* w1, const float* w2, int H, int Dp, float* wt, hipStream_t s);   // wt -> w1t, then w2t
void lstm_seq_strip_forward(const LstmSeqStrip& a, hipStream_t s);
void lstm_seq_strip_backward(const LstmSeqStrip& a, hipStream_t s);

// The critic of a recurrent rollout in one launch (lhw_mlp_strip.hip: lstm_seq_value_strip_kernel; lhw_rnn_values): one network (two stacked
// cells, read-out of ONE output) over the stored observations [T + 1][N][D] of N env rows, from and to the state lhw_rnn_forward keeps.
struct LstmSeqValues {
  const float *w1t, *w2t;                    // [in][out] copies from lstm_seq_strip_prepare
  const float *bi1, *bh1, *bi2, *bh2;        // [4H] each
  const float *wo, *bo;                      // read-out: [H], [1]
  const float *obs_mean, *obs_std;           // [D]
  const float *obs, *term_obs;               // RAW observations [T + 1][N][D], terminal observations [T][N][D] (NULL: no vterm)
  const unsigned char *done, *reset0;        // [T][N] LHW_DONE_* flags; [N] rows that start an episode at step 0 (NULL: none)
  float *h1; int h1_ld; float *h2; int h2_ld; float *c1, *c2;   // the state: rows of h1_ld / h2_ld / H floats; read, then overwritten
  float *val, *vterm, *vfinal;               // [T][N], [T][N] (with term_obs), [N] (NULL: not evaluated)
  int T, N, H, D, Dp;
};
bool lstm_seq_values_supported(int H, int Dp);   // the bounds of the other two sequence kernels
void lstm_seq_strip_values(const LstmSeqValues& a, hipStream_t s);
