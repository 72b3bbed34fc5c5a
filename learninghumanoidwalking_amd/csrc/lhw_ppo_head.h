// The PPO loss head: per-row losses and their gradients wrt the network outputs (reference rl/algos/ppo.py:302-384, FF path,
// mask = 1).  ONE definition of the arithmetic for its three callers: ppo_loss_kernel (lhw_learner.hip: a thread per row, outputs
// in HBM), mlp_train_strip_kernel (lhw_mlp_strip.hip: the row's outputs and gradients in LDS, between the forward and the backward
// layers of the same slab) and the thread-per-row kernel of lhw_debug_mlp_train_strip.
//
// Loss scalars, NSTAT per row: 0 actor_loss 1 critic_loss 2 mirror_loss 3 approx_kl 4 clip_fraction 5 imitation_loss.
// Imitation term (ppo.py:360-368): imitation_loss = mean over the selected (sample, action dim) entries of (mu - expert)^2; the
// host evaluates the env's projector and the frozen expert and hands over the dense target / mask in minibatch order
// (lhw_ppo_set_imitation); here the term enters the loss scalar and d loss / d mu.
#pragma once

#define NSTAT 6

struct LhwPpoHead {
  int B, A, Op;                               // minibatch rows (the means' denominator), action components, padded actor read-out width
  const float *act, *old_logp, *adv, *ret;    // the gathered minibatch: [B][A], [B], [B], [B]
  const float* stdv;                          // [A]
  float clip, mirror_coeff;
  int use_mirror;
  const int* act_src;                         // mirror tables [A]
  const float* act_sign;
  float* dstd;                                // [B][Op] or NULL
  const float* imit_target;                   // [B][A] or NULL
  const unsigned char* imit_mask;             // [B][A]
  float imit_coeff, imit_inv_count;
  float gscale;                               // power of two applied to the output gradients (fp16 update: loss scaling)
};

// Actor head of minibatch row m.  mu_n[0 .. A): the row's means; mu_m: those of its mirrored twin (read with use_mirror only).  Writes
// d loss / d mu to dmu_n[a * ds], a < Op, and with use_mirror the twin's to dmu_m[a * ds]; the row's dstd; s[k] = the row's term of loss
// scalar k (s[1], the critic's, is not touched).
__device__ __forceinline__ void lhw_ppo_actor_row(const LhwPpoHead& h, const int m, const float* mu_n, const float* mu_m, float* dmu_n,
                                                  float* dmu_m, const int ds, float* s) {
  const int A = h.A, Op = h.Op;
  const float* __restrict__ act = h.act;
  const float* __restrict__ stdv = h.stdv;
  const float invB = 1.f / (float)h.B, invBA = 1.f / ((float)h.B * (float)h.A);
  float s_mirror = 0, s_imit = 0;
  float lp = 0.f;
  for (int a = 0; a < A; a++) {
    float d = (act[(size_t)m * A + a] - mu_n[a]) / stdv[a];
    lp += -0.5f * d * d - logf(stdv[a]) - 0.9189385332046727f;
  }
  float logr = lp - h.old_logp[m];
  float ratio = expf(logr);
  float ad = h.adv[m];
  float cl = fminf(fmaxf(ratio, 1.f - h.clip), 1.f + h.clip);
  float cpi = ratio * ad, cll = cl * ad;
  s[0] = -fminf(cpi, cll);
  float dratio = (cpi <= cll) ? ad : 0.f;  // torch.min backward; ties inside the clip range carry the full gradient
  float dlp = -invB * dratio * ratio;
  s[3] = (ratio - 1.f) - logr;
  s[4] = fabsf(ratio - 1.f) > h.clip ? 1.f : 0.f;
  if (h.use_mirror) for (int a = 0; a < Op; a++) dmu_m[(size_t)a * ds] = 0.f;
  for (int a = 0; a < Op; a++) {
    float g = 0.f, gs = 0.f;
    if (a < A) {
      float mu = mu_n[a], sd = stdv[a], x = act[(size_t)m * A + a];
      g = dlp * (x - mu) / (sd * sd);
      gs = dlp * ((x - mu) * (x - mu) / (sd * sd * sd) - 1.f / sd);
      if (h.use_mirror) {
        // mirror_actions[a] = sign[a] * mu_mir[src[a]]  (== mu_mir @ M_a, rl/envs/wrappers.py:49-51)
        float mm = h.act_sign[a] * mu_m[h.act_src[a]];
        float diff = mu - mm;
        s_mirror += diff * diff;
        g += h.mirror_coeff * 2.f * diff * invBA;
        // gradient wrt the mirrored-pass output it came from (act_src is a permutation: each slot written once)
        dmu_m[(size_t)h.act_src[a] * ds] = -h.mirror_coeff * 2.f * diff * invBA * h.act_sign[a] * h.gscale;
      }
      if (h.imit_target && h.imit_mask[(size_t)m * A + a]) {
        float diff = mu - h.imit_target[(size_t)m * A + a];
        s_imit += diff * diff;
        g += h.imit_coeff * 2.f * diff * h.imit_inv_count;
      }
    }
    dmu_n[(size_t)a * ds] = g * h.gscale;
    if (h.dstd) h.dstd[(size_t)m * Op + a] = gs;
  }
  s[2] = s_mirror;
  s[5] = s_imit;
}

// Critic head of row m (value v): returns the row's squared error (loss scalar 1), *dv = d loss / d v
__device__ __forceinline__ float lhw_ppo_critic_row(const LhwPpoHead& h, const int m, const float v, float* dv) {
  const float invB = 1.f / (float)h.B;
  float e = h.ret[m] - v;
  *dv = -2.f * e * invB * h.gscale;
  return e * e;
}
