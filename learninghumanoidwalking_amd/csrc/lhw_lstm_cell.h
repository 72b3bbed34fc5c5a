// One hidden unit of one LSTMCell step (torch.nn.LSTMCell, gate order i f g o; the reference's Gaussian_LSTM_Actor / LSTM_V,
// rl/policies/actor.py:191-286, critic.py:52-112), shared by the stand-alone cell kernel of the launch-per-step path
// (lstm_cell_fwd_kernel, lhw_ppo.hip), the in-wave policy step of the resident rollout (lstm_policy_step, lhw_humanoid_rollout.hip)
// and its plain reference launch (lhw_debug_lstm_policy_step, lhw_mlp_strip.hip).  One definition, so all three produce the same bits.
//
// Those translation units are compiled with different -ffp-contract settings (lhw_ppo.hip and lhw_mlp_strip.hip with hipcc's default,
// fast, where the back end decides which multiply feeds which add; the stepper units with `on`), so every multiply-add is spelled out:
// the cell update is the form the back end chose for `gf * cp + gi * gg` in lstm_cell_fwd_kernel before this header existed --
// the product gf * cp rounded on its own, then one fused gi * gg + (gf * cp) -- and nothing is left for the contraction to decide.
#pragma once
#include <math.h>

#include "lhw_rng.h"   // LHW_HD

LHW_HD float lhw_sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

// g_*: the four gate pre-activations of the unit as the GEMM over [x | h_prev] left them (biases not yet added); b_ih / b_hh: the
// unit's entries of the two bias vectors per gate, in gate order i f g o.  The activated gates go to gates[0..3] (the backward pass
// reads them), the new cell state to *c; returns the new hidden state.
LHW_HD float lhw_lstm_cell(float g_i, float g_f, float g_g, float g_o, const float b_ih[4], const float b_hh[4], float c_prev, float gates[4], float* c) {
  const float gi = lhw_sigmoidf((g_i + b_ih[0]) + b_hh[0]);
  const float gf = lhw_sigmoidf((g_f + b_ih[1]) + b_hh[1]);
  const float gg = tanhf((g_g + b_ih[2]) + b_hh[2]);
  const float go = lhw_sigmoidf((g_o + b_ih[3]) + b_hh[3]);
  const float fc = gf * c_prev;            // (a product on its own: no addition follows it in this expression)
  const float cn = fmaf(gi, gg, fc);
  gates[0] = gi; gates[1] = gf; gates[2] = gg; gates[3] = go;
  *c = cn;
  return go * tanhf(cn);
}
