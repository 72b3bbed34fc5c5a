// What the feed-forward and the recurrent PPO learner share: the handle core, the loss / statistics kernels, dual grad-norm clip +
// Adam, and the handle-free advantage entries.  Takes over the arithmetic of
//   PPOBuffer.finish_path (GAE)           (reference rl/storage/rollout_storage.py:53-85)
//   the losses of PPO.update_actor_critic (reference rl/algos/ppo.py:299-406), per row in lhw_ppo_head.h
//   advantage normalisation               (reference rl/algos/ppo.py:484-485)
// GAE accumulates in float64 like the reference.
#include "lhw_learner.h"

#include <cmath>
#include <mutex>
#include <vector>

#include "lhw_policy.h"
#include "lhw_rng.h"

// (x - mean)/std into a [R][Dp] buffer (pad columns zero); optional mirrored copy
// mirror: out[j] = sign[j] * obs[src[j]]  == obs @ M with the clock sign flip folded in
// (reference rl/envs/wrappers.py:53-85: sin(arcsin(c)+pi) == -c)
__global__ void normalize_kernel(const float* __restrict__ obs, int D, int Dp, size_t R, const float* __restrict__ mean,
                                 const float* __restrict__ stdv, float* __restrict__ xn, float* __restrict__ xm,
                                 const int* __restrict__ src, const float* __restrict__ sign) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= R * (size_t)Dp) return;
  size_t r = i / Dp;
  int j = (int)(i - r * Dp);
  float v = 0.f, vm = 0.f;
  if (j < D) {
    v = (obs[r * D + j] - mean[j]) / stdv[j];
    if (xm) vm = (sign[j] * obs[r * D + src[j]] - mean[j]) / stdv[j];
  }
  xn[i] = v;
  if (xm) xm[i] = vm;
}
// rollout sampling: act = mu + std * N(0,1) (or mu), logp of the sampled action under (mu, std)
// One (row, action component) per lane, 32 lanes per row (act_dim <= 32): the Box-Muller draw is ~400 instructions of float64
// transcendentals per component, so a thread per row (12 draws in sequence, 8 blocks for a 2048-row group) left this kernel
// latency-bound at 15 us on the rollout's critical path.  The log-density terms are summed by the row's first lane in
// component order, as the fused read-out of the forward strip kernel does (bit-identical log-probabilities).
__global__ void __launch_bounds__(256) sample_kernel(const float* __restrict__ mu, int ldmu, int A, int N, const float* __restrict__ stdv,
                                                     uint64_t seed, uint32_t env_base, uint32_t counter, int deterministic,
                                                     float* __restrict__ act, float* __restrict__ logp) {
  __shared__ float terms[8][32];
  LHW_LDS_POISON(terms);
  const int r = threadIdx.x >> 5, a = threadIdx.x & 31, n = blockIdx.x * 8 + r;
  if (n < N && a < A) {
    float term;
    act[(size_t)n * A + a] = lhw_policy_sample(mu[(size_t)n * ldmu + a], stdv[a], seed, env_base + n, counter, a, deterministic, &term);
    terms[r][a] = term;
  }
  __syncthreads();
  if (n < N && a == 0) {
    float lp = 0.f;
    for (int k = 0; k < A; k++) lp += terms[r][k];
    logp[n] = lp;
  }
}
// PPO losses and their gradients wrt network outputs: the per-row arithmetic is lhw_ppo_head.h's, here a thread per row on outputs
// in HBM.  No atomics: bias / std gradients are column sums of dya / dyc / dstd taken afterwards in a fixed order, and the loss
// scalars are written as per-block partials [gridDim.x][NSTAT] (clip_fraction already divided by B).
// block reduction of the row terms (already scaled) in a fixed order: xor butterfly inside the wave, then waves 0..3
__device__ __forceinline__ void ppo_stats_block(float (&vals)[NSTAT], float* __restrict__ stats_part) {
  __shared__ float red[NSTAT][4];
  LHW_LDS_POISON(red);
  for (int o = 32; o > 0; o >>= 1)
    for (int k = 0; k < NSTAT; k++) vals[k] += __shfl_xor(vals[k], o);
  int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0)
    for (int k = 0; k < NSTAT; k++) red[k][wave] = vals[k];
  __syncthreads();
  if (threadIdx.x < NSTAT) stats_part[(size_t)blockIdx.x * NSTAT + threadIdx.x] = (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
}
__global__ void __launch_bounds__(256) ppo_loss_kernel(int B, int Rcap, int A, int Op, const float* __restrict__ ya,
                                                       const float* __restrict__ yc, const float* __restrict__ act,
                                                       const float* __restrict__ old_logp, const float* __restrict__ adv,
                                                       const float* __restrict__ ret, const float* __restrict__ stdv,
                                                       float clip, float mirror_coeff, int use_mirror,
                                                       const int* __restrict__ act_src, const float* __restrict__ act_sign,
                                                       float* __restrict__ dya, float* __restrict__ dyc,
                                                       float* __restrict__ dstd /* [B][Op] or NULL */, float* __restrict__ stats_part,
                                                       const float* __restrict__ imit_target /* [B][A] or NULL */,
                                                       const unsigned char* __restrict__ imit_mask /* [B][A] */, float imit_coeff,
                                                       float imit_inv_count, int seqB,
                                                       float gscale /* power of two applied to dya / dyc (fp16 update: loss scaling) */) {
  int m = blockIdx.x * blockDim.x + threadIdx.x;
  // row of sample m in the actor output buffer, and of its mirrored twin: FF minibatch: m and Rcap + m; recurrent minibatch
  // (time-major, seqB columns per step, mirrored columns appended per step): t * 2 seqB + b and + seqB
  size_t rn = (size_t)m, rm = (size_t)Rcap + m;
  if (seqB > 0 && use_mirror) { rn = (size_t)(m / seqB) * (2 * (size_t)seqB) + (size_t)(m % seqB); rm = rn + seqB; }
  const LhwPpoHead h{B, A, Op, act, old_logp, adv, ret, stdv, clip, mirror_coeff, use_mirror, act_src, act_sign, dstd, imit_target, imit_mask,
                     imit_coeff, imit_inv_count, gscale};
  float t[NSTAT] = {0, 0, 0, 0, 0, 0};
  const float invB = 1.f / (float)B, invBA = 1.f / ((float)B * (float)A);
  if (m < B) {
    lhw_ppo_actor_row(h, m, ya + rn * Op, ya + rm * Op, dya + rn * Op, dya + rm * Op, 1, t);
    float dv;
    t[1] = lhw_ppo_critic_row(h, m, yc[(size_t)m * 4], &dv);
    dyc[(size_t)m * 4] = dv;
    dyc[(size_t)m * 4 + 1] = 0.f; dyc[(size_t)m * 4 + 2] = 0.f; dyc[(size_t)m * 4 + 3] = 0.f;
  }
  float vals[NSTAT] = {t[0] * invB, t[1] * invB, t[2] * invBA, t[3] * invB, t[4] * invB, t[5] * imit_inv_count};
  ppo_stats_block(vals, stats_part);
}

// The loss scalars of a step whose heads ran inside the train strip kernels: those leave every row's terms in rows [NSTAT][ld] (term-major);
// the same per-block partials as ppo_loss_kernel's, from the same values in the same order
__global__ void __launch_bounds__(256) ppo_stats_rows_kernel(int B, int A, const float* __restrict__ rows, int ld, float imit_inv_count,
                                                             float* __restrict__ stats_part) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  float t[NSTAT] = {0, 0, 0, 0, 0, 0};
  if (m < B)
    for (int k = 0; k < NSTAT; k++) t[k] = rows[(size_t)k * ld + m];
  const float invB = 1.f / (float)B, invBA = 1.f / ((float)B * (float)A);
  float vals[NSTAT] = {t[0] * invB, t[1] * invB, t[2] * invBA, t[3] * invB, t[4] * invB, t[5] * imit_inv_count};
  ppo_stats_block(vals, stats_part);
}

// out[k] += sum_b part[b][n] in block order (single block; n small)
__global__ void reduce_rows_kernel(const float* __restrict__ part, int nrows, int n, float* __restrict__ out) {
  int k = threadIdx.x;
  if (k >= n) return;
  float s = 0.f;
  for (int b = 0; b < nrows; b++) s += part[(size_t)b * n + k];
  out[k] += s;
}

// entropy_penalty = -mean(entropy) = -mean_a(0.5 + 0.5 log 2pi + log std_a): d/d std_a = -1/(A std_a) (ppo.py:343,380)
__global__ void entropy_grad_kernel(const float* __restrict__ stdv, int A, float ent_coeff, float* __restrict__ grad_std) {
  int a = threadIdx.x;
  if (a < A) grad_std[a] += -ent_coeff / ((float)A * stdv[a]);
}
// sum of squares of a flat range (grad norm), with pre-scale: per-block partials (fixed grid), summed in block order
// clip_grad_norm_ (coef = max_norm/(norm+1e-6), applied only if < 1) + torch.optim.Adam step; zeroes the gradient
// The two parameter groups (actor [+ stds], critic) in two launches instead of six: the per-block sums of squares of both groups
// from one grid, and one Adam grid over both groups whose blocks each add their group's SUMSQ_BLOCKS partials in the order
// sumsq_final_kernel used (same bits), instead of waiting for a one-thread launch per group to do it.
__global__ void __launch_bounds__(256) sumsq2_kernel(const float* __restrict__ g0, size_t n0, const float* __restrict__ g1, size_t n1, float scale,
                                                     float* __restrict__ part /* [2][SUMSQ_BLOCKS] */) {
  const int grp = blockIdx.x / SUMSQ_BLOCKS, b = blockIdx.x - grp * SUMSQ_BLOCKS;
  const float* __restrict__ g = grp ? g1 : g0;
  const size_t n = grp ? n1 : n0;
  float s = 0.f;
  for (size_t i = (size_t)b * blockDim.x + threadIdx.x; i < n; i += (size_t)SUMSQ_BLOCKS * blockDim.x) {
    float v = g[i] * scale;
    s += v * v;
  }
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  __shared__ float red[4];
  LHW_LDS_POISON(red);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ void __launch_bounds__(256) adam2_kernel(AdamArgs a) {
  float *__restrict__ theta = a.theta, *__restrict__ grad = a.grad, *__restrict__ m = a.m, *__restrict__ v = a.v, *__restrict__ normsq_out = a.normsq_out;
  const float* __restrict__ part = a.part;
  const size_t n0 = a.n0, off1 = a.off1, n1 = a.n1;
  const int blocks0 = a.blocks0;
  const float gscale = a.gscale, max_norm = a.max_norm, lr = a.lr, beta1 = a.beta1, beta2 = a.beta2, eps = a.eps, bc1 = a.bc1, bc2sqrt = a.bc2sqrt;
  const int grp = (int)blockIdx.x >= blocks0 ? 1 : 0;
  __shared__ float nsq;
  LHW_LDS_POISON(nsq);
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int b = 0; b < SUMSQ_BLOCKS; b++) s += part[grp * SUMSQ_BLOCKS + b];
    nsq = s;
    if ((int)blockIdx.x == (grp ? blocks0 : 0)) normsq_out[grp] = s;
  }
  __syncthreads();
  const size_t i = (size_t)((int)blockIdx.x - (grp ? blocks0 : 0)) * blockDim.x + threadIdx.x;
  if (i >= (grp ? n1 : n0)) return;
  const size_t e = (grp ? off1 : 0) + i;
  float norm = sqrtf(nsq);
  float coef = max_norm / (norm + 1e-6f);
  coef = coef < 1.f ? coef : 1.f;
  float g = grad[e] * gscale * coef;
  float mi = beta1 * m[e] + (1.f - beta1) * g;
  float vi = beta2 * v[e] + (1.f - beta2) * g * g;
  m[e] = mi; v[e] = vi;
  float denom = sqrtf(vi) / bc2sqrt + eps;
  theta[e] -= (lr / bc1) * (mi / denom);
  grad[e] = 0.f;
}
// GAE(lambda) over a time-major rollout, one lane per env, float64 accumulation
// (reference rl/storage/rollout_storage.py:53-85 + the bootstrap rules of rl/workers/rollout_worker.py:163-190)
__global__ void __launch_bounds__(256) gae_kernel(int T, int N, const float* __restrict__ rew, const float* __restrict__ val,
                                                  const uint8_t* __restrict__ done, const float* __restrict__ vterm,
                                                  const float* __restrict__ vfinal, double gamma, double lam,
                                                  float* __restrict__ ret, float* __restrict__ adv) {
  int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  double gae = 0.0, nextv = (double)vfinal[n];
  for (int t = T - 1; t >= 0; t--) {
    size_t i = (size_t)t * N + n;
    uint8_t f = done[i];
    if (f) {  // trajectory ends here: bootstrap (not done) * V(terminal obs), advantage recursion restarts
      nextv = (f & 1) ? 0.0 : (double)vterm[i];
      gae = 0.0;
    }
    double v = (double)val[i];
    double delta = (double)rew[i] + gamma * nextv - v;
    gae = delta + gamma * lam * gae;
    double r = gae + v;
    ret[i] = (float)r;
    adv[i] = (float)r - val[i];  // advantages = returns.float() - values.float() (ppo.py:484)
    nextv = v;
  }
}

// advantage normalisation: (a - mean) / (std_unbiased + eps) from global moments
#define MOM_BLOCKS 256
__global__ void __launch_bounds__(256) moments_kernel(const float* __restrict__ x, size_t n, double* __restrict__ part) {
  double s = 0, s2 = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    double v = x[i];
    s += v; s2 += v * v;
  }
  for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o); s2 += __shfl_xor(s2, o); }
  __shared__ double red[2][4];
  LHW_LDS_POISON(red);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = s; red[1][threadIdx.x >> 6] = s2; }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    part[2 * blockIdx.x + 1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  }
}
__global__ void moments_final_kernel(const double* __restrict__ part, int n, double* __restrict__ out) {
  if (threadIdx.x < 2) {
    double s = 0;
    for (int b = 0; b < n; b++) s += part[2 * b + threadIdx.x];
    out[threadIdx.x] = s;
  }
}
__global__ void scale_shift_kernel(float* __restrict__ x, size_t n, float mean, float inv) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) x[i] = (x[i] - mean) * inv;
}

// x <- (x - mean) / (std + eps) with mean / UNBIASED std formed on the device from (sum, sum of squares, count) -- the same double
// arithmetic, rounded to float32 at the same point, as the host path of lhw_scale_shift's callers (global_mean_std)
__global__ void standardize_kernel(float* __restrict__ x, size_t n, const double* __restrict__ st, double eps) {
  const double cnt = st[2], mean = st[0] / cnt;
  const double var = fmax(0.0, (st[1] - cnt * mean * mean) / fmax(1.0, cnt - 1.0));
  const float mean_f = (float)mean, inv_f = (float)(1.0 / (sqrt(var) + eps));
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) x[i] = (x[i] - mean_f) * inv_f;
}
// ------------------------------------------------------------------------------------------- the learner core
int learner_check(const LhwPpoConfig* c, void** out, bool caps_ok) {
  if (!c || !out) return lhw_fail(LHW_ERR_ARG, "null argument");
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return lhw_fail(LHW_ERR_NO_DEVICE, "no HIP device visible: liblhw has no CPU fallback");
  if (c->obs_dim <= 0 || c->act_dim <= 0 || c->act_dim > 32 || c->hidden <= 0 || c->hidden % 4 || !caps_ok)
    return lhw_fail(LHW_ERR_ARG, "bad PPO dimensions (act_dim <= 32, hidden %% 4 == 0, capacities > 0)");
  HIPCHK(hipSetDevice(c->device));
  return LHW_OK;
}
void learner_init(LearnerCore& k, const LhwPpoConfig* c, size_t n_actor, size_t n_critic) {
  k.device = k.mem.device = c->device; k.D = c->obs_dim; k.Dp = pad4(k.D); k.A = c->act_dim; k.H = c->hidden; k.learn_std = c->learn_std;
  k.clip = c->clip; k.ent_coeff = c->entropy_coeff; k.mirror_coeff = c->mirror_coeff; k.grad_clip = c->max_grad_norm;
  k.lr = c->lr; k.adam_eps = c->eps; k.beta1 = 0.9f; k.beta2 = 0.999f;
  k.use_mirror = c->mirror_obs_src != nullptr;
  k.off_actor = 0; k.off_std = n_actor; k.off_critic = k.off_std + pad4(k.A); k.n_critic = n_critic; k.n_params = k.off_critic + n_critic;
}
bool learner_mirror(LearnerCore& k, const LhwPpoConfig* c) {
  if (!k.use_mirror) return true;
  std::vector<int> osrc(k.Dp, 0), asrc(k.A, 0);
  std::vector<float> osgn(k.Dp, 0.f), asgn(k.A, 0.f);
  for (int j = 0; j < k.D; j++) { osrc[j] = c->mirror_obs_src[j]; osgn[j] = c->mirror_obs_sign[j]; if (osrc[j] < 0 || osrc[j] >= k.D) return false; }
  for (int j = 0; j < k.A; j++) { asrc[j] = c->mirror_act_src[j]; asgn[j] = c->mirror_act_sign[j]; if (asrc[j] < 0 || asrc[j] >= k.A) return false; }
  k.d_obs_src = k.mem.put(osrc.data(), osrc.size()); k.d_act_src = k.mem.put(asrc.data(), asrc.size());
  k.d_obs_sign = k.mem.put(osgn.data(), osgn.size()); k.d_act_sign = k.mem.put(asgn.data(), asgn.size());
  return !k.mem.failed();
}
int learner_normalize(LearnerCore* k, const float* obs, int64_t R, const float* obs_mean, const float* obs_std, float* xn, float* xm,
                             void* stream) {
  if (!k || !obs || !xn || R <= 0) return lhw_fail(LHW_ERR_ARG, "bad argument");
  if (xm && !k->use_mirror) return lhw_fail(LHW_ERR_ARG, "mirror output requested but no mirror tables configured");
  HIPCHK(hipSetDevice(k->device));
  size_t n = (size_t)R * k->Dp;
  hipLaunchKernelGGL(normalize_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, obs, k->D, k->Dp, (size_t)R,
                     obs_mean, obs_std, xn, xm, k->d_obs_src, k->d_obs_sign);
  HIPCHK(hipGetLastError());
  return LHW_OK;
}
#define LHW_MAX_DEVICES 64
// device that owns a device pointer; makes it current (the handle-free entry points below have no LhwPpo to ask)
static int device_of(const void* ptr, int* dev) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, ptr) != hipSuccess) return lhw_fail(LHW_ERR_ARG, "not a device pointer");
  if (at.device < 0 || at.device >= LHW_MAX_DEVICES) return lhw_fail(LHW_ERR_ARG, "device %d out of range", at.device);
  if (hipSetDevice(at.device) != hipSuccess) return lhw_fail(LHW_ERR_HIP, "hipSetDevice(%d) failed", at.device);
  *dev = at.device;
  return 0;
}

extern "C" int lhw_gae(int32_t T, int32_t N, const float* rew, const float* val, const uint8_t* done, const float* vterm,
                       const float* vfinal, double gamma, double lam, float* ret, float* adv, void* stream) {
  if (T <= 0 || N <= 0 || !rew || !val || !done || !vterm || !vfinal || !ret || !adv) return lhw_fail(LHW_ERR_ARG, "bad argument");
  int dev = 0;
  if (device_of(rew, &dev)) return LHW_ERR_HIP;
  hipLaunchKernelGGL(gae_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, T, N, rew, val, done, vterm, vfinal,
                     gamma, lam, ret, adv);
  HIPCHK(hipGetLastError());
  return LHW_OK;
}

// sum and sum of squares (float64) of x[0..n): the caller all-reduces them across GPUs, then calls lhw_scale_shift
extern "C" int lhw_moments(const float* x, int64_t n, double* out2_dev, void* stream) {
  if (!x || !out2_dev || n <= 0) return lhw_fail(LHW_ERR_ARG, "bad argument");
  // handle-free entry point: run on the device that owns x, with that device's own partial-sum buffer (kept for the
  // process lifetime; one per device, so a process driving several GPUs never hands a kernel a foreign-device pointer)
  int dev = 0;
  if (device_of(x, &dev)) return LHW_ERR_HIP;
  static double* scratch_of[LHW_MAX_DEVICES] = {nullptr};   // (shared by the streams of a device: a behaviour question, left as it is)
  static std::mutex mu;
  double* scratch;
  {
    std::lock_guard<std::mutex> lock(mu);
    if (!scratch_of[dev]) HIPCHK(lhw_malloc(&scratch_of[dev], sizeof(double) * 2 * MOM_BLOCKS));
    scratch = scratch_of[dev];
  }
  hipLaunchKernelGGL(moments_kernel, dim3(MOM_BLOCKS), dim3(256), 0, (hipStream_t)stream, x, (size_t)n, scratch);
  hipLaunchKernelGGL(moments_final_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, scratch, MOM_BLOCKS, out2_dev);
  HIPCHK(hipGetLastError());
  return LHW_OK;
}
extern "C" int lhw_scale_shift(float* x, int64_t n, float mean, float inv_scale, void* stream) {
  if (!x || n <= 0) return lhw_fail(LHW_ERR_ARG, "bad argument");
  int dev = 0;
  if (device_of(x, &dev)) return LHW_ERR_HIP;
  hipLaunchKernelGGL(scale_shift_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, x, (size_t)n, mean, inv_scale);
  HIPCHK(hipGetLastError());
  return LHW_OK;
}

extern "C" int lhw_standardize(float* x, int64_t n, const double* stats3_dev, double eps, void* stream) {
  if (!x || !stats3_dev || n <= 0) return lhw_fail(LHW_ERR_ARG, "bad argument");
  int dev = 0;
  if (device_of(x, &dev)) return LHW_ERR_HIP;
  hipLaunchKernelGGL(standardize_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, x, (size_t)n, stats3_dev, eps);
  HIPCHK(hipGetLastError());
  return LHW_OK;
}
// dual clip_grad_norm_ + Adam on the two parameter groups [0, na) and [off_critic, off_critic + n_critic) of the flat vector; na: the actor
// group (+ stds if they are parameters)
AdamArgs learner_adam_args(const LearnerCore& k, float* theta, float* grad, float* adam_m, float* adam_v, int64_t step, float grad_scale) {
  const size_t na = k.learn_std ? k.off_std + k.A : k.off_std;
  const float bc1 = 1.f - powf(k.beta1, (float)step), bc2 = 1.f - powf(k.beta2, (float)step);
  return AdamArgs{theta, grad, adam_m, adam_v, na, k.off_critic, k.n_critic, (int)((na + 255) / 256), grad_scale, k.norm_part, k.stats + 8,
                  k.grad_clip, k.lr, k.beta1, k.beta2, k.adam_eps, bc1, sqrtf(bc2)};
}
static void clip_and_adam(const AdamArgs& a, hipStream_t s) {
  const int blocks1 = (int)((a.n1 + 255) / 256);
  hipLaunchKernelGGL(sumsq2_kernel, dim3(2 * SUMSQ_BLOCKS), dim3(256), 0, s, a.grad, a.n0, a.grad + a.off1, a.n1, a.gscale, a.part);
  hipLaunchKernelGGL(adam2_kernel, dim3(a.blocks0 + blocks1), dim3(256), 0, s, a);
}

int learner_apply(LearnerCore* k, float* theta, float* grad, float* adam_m, float* adam_v, int64_t step, float grad_scale, void* stream) {
  if (!k || !theta || !grad || !adam_m || !adam_v || step <= 0) return lhw_fail(LHW_ERR_ARG, "bad argument");
  HIPCHK(hipSetDevice(k->device));
  hipStream_t s = (hipStream_t)stream;
  clip_and_adam(learner_adam_args(*k, theta, grad, adam_m, adam_v, step, grad_scale), s);
  if (!k->learn_std) HIPCHK(hipMemsetAsync(grad + k->off_std, 0, sizeof(float) * pad4(k->A), s));
  HIPCHK(hipGetLastError());
  return LHW_OK;
}

// Test hook: waits for the device, then copies the two squared gradient norms (actor group, critic group; after grad_scale, before
// clipping) that the last lhw_ppo_apply / lhw_ppo_step / lhw_rnn_apply wrote into stats[8..9] to the host
int learner_grad_sqnorms(LearnerCore* k, float* out2_host) {
  if (!k || !out2_host) return lhw_fail(LHW_ERR_ARG, "null argument");
  HIPCHK(hipSetDevice(k->device));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(out2_host, k->stats + 8, 2 * sizeof(float), hipMemcpyDeviceToHost));
  return LHW_OK;
}
