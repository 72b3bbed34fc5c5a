// The fp16 strip kernels (lhw_mlp_strip_h.hip) as the feed-forward learner calls them: the forward and the backward pass of one 3-layer MLP
// with fp16 operands, one launch each -- bit for bit three / two gemm_h_kernel launches with fp16 storage.  Narrow shapes only
// (mlp_strip_h_supported).  They multiply by fp16 copies of the float32 master weights in the MFMA's operand order, made by
// mlp_strip_h_prepare whenever theta has changed (once per optimiser step / rollout bracket / forward call): the same rounding the GEMMs apply
// while they stage the weights, done once instead of once per slab.
#pragma once
#include <hip/hip_runtime.h>

#define MLP_STRIP_H_WH_HALVES 163840         // halves of one network's copies (every shape: the regions are sized for the capacities)
void mlp_strip_h_prepare(const float* w1, const float* w2, const float* w3, int Dp, int O, _Float16* wh, hipStream_t s);   // torch layout in: W1 [256][Dp], W2 [256][256], W3 [>= O][256]
struct MlpStripFwdH {
  const _Float16* wh;                        // the network's READY copies
  const float *b1, *b2, *b3;                 // biases, float32
  const float* x; int ldx;                   // float32 inputs [R][ldx], rounded while staged (inference) -- or, x == NULL,
  const _Float16* x_h; int ldxh;             // fp16 inputs [R][ldxh] (the update)
  int Dp, O, Op, R;
  _Float16 *h1_h, *h2_h;                     // [R][256] each, 16-byte aligned; NULL: not written to HBM
  float* y;                                  // [R][Op], columns < O written
};
struct MlpStripBwdH {
  const _Float16* wh;
  const float* dy;                           // [R][Op] float32, rounded while staged
  const _Float16 *h1_h, *h2_h;               // the forward pass's stored activations: the ReLU masks (> 0)
  int O, Op, R;
  _Float16 *dh2_h, *dh1_h;                   // [R][256] each, 16-byte aligned
};
bool mlp_strip_h_supported(int H, int Dp, int O, int Op);   // hidden 256, Dp <= 64 (a multiple of 4), O <= 32: mlp_strip_supported's shapes
void mlp_strip_forward_h(const MlpStripFwdH& a, hipStream_t s);
void mlp_strip_backward_h(const MlpStripBwdH& a, hipStream_t s);
