// What the feed-forward learner (lhw_ppo.hip) and the recurrent learner (lhw_rnn.hip) do the same way (lhw_learner.hip): the handle's
// core, its create / normalise / apply steps, the loss and statistics kernels both launch, and the clip + Adam step.
#pragma once
#include "lhw_internal.h"

// Shapes, hyper-parameters, the groups of the flat parameter vector [actor | stds(A, padded to 4) | critic], the mirror tables, the
// loss / optimiser scratch -- and the owner of the handle's device memory.  learner_* are the operations that read nothing else.
struct LearnerCore {
  int device = 0, D = 0, Dp = 0, A = 0, H = 0, learn_std = 0;   // Dp = pad4(D)
  float clip, ent_coeff, mirror_coeff, grad_clip, lr, adam_eps, beta1, beta2;
  int use_mirror = 0;
  size_t off_actor = 0, off_std = 0, off_critic = 0, n_critic = 0, n_params = 0;   // n_critic: parameters of the critic group
  // mirror tables (device): obs_src[Dp], obs_sign[Dp], act_src[A], act_sign[A]
  int *d_obs_src = nullptr, *d_act_src = nullptr;
  float *d_obs_sign = nullptr, *d_act_sign = nullptr;
  float *stats = nullptr;       // [16] loss scalars; [8],[9] grad norm^2 actor/critic
  float *stats_part = nullptr;  // per-block loss partials [blocks][NSTAT]
  float *norm_part = nullptr;   // [2][SUMSQ_BLOCKS]
  LhwDevMem mem;
};
#define SUMSQ_BLOCKS 128

// the checks of a create call, before it touches the device (caps_ok: the handle's own capacities are positive); clears *out
int learner_check(const LhwPpoConfig* c, void** out, bool caps_ok);
void learner_init(LearnerCore& k, const LhwPpoConfig* c, size_t n_actor, size_t n_critic);
// checks the mirror tables of the config and uploads them (no-op without); false: an index out of range (or a failed allocation: k.mem)
bool learner_mirror(LearnerCore& k, const LhwPpoConfig* c);
// normalised (and mirrored) copies of R raw observation rows: xn/xm [R][Dp]
int learner_normalize(LearnerCore* k, const float* obs, int64_t R, const float* obs_mean, const float* obs_std, float* xn, float* xm, void* stream);
// clip_grad_norm_ on the actor and critic parameter groups separately, then one Adam step each; zeroes grad.
// grad_scale multiplies the gradient first (1/world_size after a sum all-reduce).  step is the 1-based Adam step count.
int learner_apply(LearnerCore* k, float* theta, float* grad, float* adam_m, float* adam_v, int64_t step, float grad_scale, void* stream);
int learner_grad_sqnorms(LearnerCore* k, float* out2_host);

// adam2_kernel's argument: learner_apply launches it with what learner_adam_args returns, and so does whoever patches a captured launch
struct AdamArgs {
  float *theta, *grad, *m, *v;
  size_t n0, off1, n1;      // the two parameter groups [0, n0) and [off1, off1 + n1)
  int blocks0;
  float gscale;
  float* part;              // [2][SUMSQ_BLOCKS]: sumsq2_kernel writes it, adam2_kernel reads it
  float* normsq_out;        // [2]
  float max_norm, lr, beta1, beta2, eps, bc1, bc2sqrt;
};
AdamArgs learner_adam_args(const LearnerCore& k, float* theta, float* grad, float* adam_m, float* adam_v, int64_t step, float grad_scale);
__global__ void adam2_kernel(AdamArgs a);

// The critic's chain runs on a side stream beside the actor's: sc waits for s at fork(), s for sc at join() (sc == s: one stream, no-ops)
struct StreamPair {
  hipStream_t s, sc;
  hipEvent_t ev_fork, ev_join;
  void fork() const { if (sc != s) { (void)hipEventRecord(ev_fork, s); (void)hipStreamWaitEvent(sc, ev_fork, 0); } }
  void join() const { if (sc != s) { (void)hipEventRecord(ev_join, sc); (void)hipStreamWaitEvent(s, ev_join, 0); } }
};

// kernels both learners launch (definitions and comments: lhw_learner.hip)
__global__ void normalize_kernel(const float* __restrict__ obs, int D, int Dp, size_t R, const float* __restrict__ mean, const float* __restrict__ stdv,
                                 float* __restrict__ xn, float* __restrict__ xm, const int* __restrict__ src, const float* __restrict__ sign);
__global__ void sample_kernel(const float* __restrict__ mu, int ldmu, int A, int N, const float* __restrict__ stdv, uint64_t seed, uint32_t env_base,
                              uint32_t counter, int deterministic, float* __restrict__ act, float* __restrict__ logp);
__global__ void ppo_loss_kernel(int B, int Rcap, int A, int Op, const float* __restrict__ ya, const float* __restrict__ yc, const float* __restrict__ act,
                                const float* __restrict__ old_logp, const float* __restrict__ adv, const float* __restrict__ ret,
                                const float* __restrict__ stdv, float clip, float mirror_coeff, int use_mirror, const int* __restrict__ act_src,
                                const float* __restrict__ act_sign, float* __restrict__ dya, float* __restrict__ dyc, float* __restrict__ dstd,
                                float* __restrict__ stats_part, const float* __restrict__ imit_target, const unsigned char* __restrict__ imit_mask,
                                float imit_coeff, float imit_inv_count, int seqB, float gscale);
__global__ void ppo_stats_rows_kernel(int B, int A, const float* __restrict__ rows, int ld, float imit_inv_count, float* __restrict__ stats_part);
__global__ void reduce_rows_kernel(const float* __restrict__ part, int nrows, int n, float* __restrict__ out);
__global__ void entropy_grad_kernel(const float* __restrict__ stdv, int A, float ent_coeff, float* __restrict__ grad_std);
