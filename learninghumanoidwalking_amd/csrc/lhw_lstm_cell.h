// One hidden unit of one LSTMCell step (torch.nn.LSTMCell, gate order i f g o; the reference's Gaussian_LSTM_Actor / LSTM_V,
// rl/policies/actor.py:191-286, critic.py:52-112), shared by the stand-alone cell kernel of the launch-per-step path
// (lstm_cell_fwd_kernel, lhw_lstm_steps.h), the in-wave policy step of the resident rollout (lstm_policy_step, lhw_humanoid_rollout.hip)
// and its plain reference launch (lhw_debug_lstm_policy_step, lhw_mlp_strip.hip), and by the whole-sequence strip kernels of the recurrent update
// (lstm_seq_fwd_strip_kernel / lstm_seq_bwd_strip_kernel, lhw_mlp_strip.hip).  One definition, so all of them produce the same bits.
//
// Those translation units are compiled with different -ffp-contract settings (lhw_rnn.hip and lhw_mlp_strip.hip with hipcc's default,
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

// Backward of one hidden unit of one cell step (BPTT of the recurrent update: lstm_cell_bwd_kernel of the launch-per-step path, lhw_lstm_steps.h,
// and lstm_seq_bwd_strip_kernel, lhw_mlp_strip.hip).  gates: the unit's activated gates i f g o of step t; c: its cell state of step t;
// c_prev: of step t - 1 (0 at t = 0); reset_t: an episode starts at step t (the state before it was zero, and nothing is carried across it);
// dh_a: d loss / d h_t from the layer above at step t; dh_b: from this cell's own recurrent input at step t + 1, which counts unless
// reset_next (the last step, or step t + 1 starts an episode: its recurrent input was zeroed).  *dcar: d loss / d c carried from step t + 1
// in, to step t - 1 out.  d[0..3]: d loss / d pre-activation of the four gates.
// The roundings are the ones the back end chose for the expressions that stood in lstm_cell_bwd_kernel before this function existed
// (tc * tc rounded on its own and subtracted from 1; dct and 1 - gg * gg fused; every other product rounded left to right), spelled out and
// with contraction switched off inside the function, so that no kernel's surroundings can change them.
LHW_HD void lhw_lstm_cell_bwd(const float gates[4], float c, float c_prev, bool reset_t, float dh_a, float dh_b, bool reset_next, float* dcar, float d[4]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float gi = gates[0], gf = gates[1], gg = gates[2], go = gates[3];
  const float cp = reset_t ? 0.f : c_prev;
  float dh = dh_a;
  if (!reset_next) dh += dh_b;
  const float tc = tanhf(c);
  const float t2 = tc * tc;
  const float dct = fmaf(dh * go, 1.f - t2, *dcar);
  *dcar = reset_t ? 0.f : dct * gf;
  d[0] = ((dct * gg) * gi) * (1.f - gi);
  d[1] = ((dct * cp) * gf) * (1.f - gf);
  d[2] = (dct * gi) * fmaf(-gg, gg, 1.f);
  d[3] = ((dh * tc) * go) * (1.f - go);
}
