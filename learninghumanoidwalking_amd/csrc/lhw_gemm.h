// The dense kernels of the update (lhw_gemm.hip) as the learners call them: the MFMA GEMM with its fused epilogues, the ordered
// reductions of split-K partials and column sums, and the two K-streaming weight-gradient kernels.
#pragma once
#include <hip/hip_runtime.h>

struct GemmArgs {
  const float* A; int lda;
  const float* B; int ldb;
  float* C; int ldc;
  int M, N, K;
  const float* bias;        // + bias[n]
  int relu;                 // max(0, .)
  const float* mask; int ldmask;  // *= (mask[m][n] > 0)
  float* part;              // split-K: slice z stores its partial product at part + z*M*N (row-major, ld N); reduced in slice order afterwards
  int k_chunk;              // K range per blockIdx.z
  float* colsum;            // (A stored [K][M] only) slice z also stores sum_k A[k][m] at colsum + z*M: the bias gradient of a dW GEMM
  int tiles_m, tiles_n, slices;   // filled in by launch_gemm
  // fp16 GEMM only (gemm_h_kernel): which of the buffers hold _Float16 instead of float (the pointers above are then reinterpreted;
  // leading dimensions count elements of the buffer's own type).  Operands stored as float are rounded to fp16 while they are staged.
  int a_half, b_half, c_half, mask_half;
};
// C = op(A) op(B).  A_KC: A is stored [M][K] (K contiguous), else [K][M]; B_KC: B is stored [N][K], else [K][N].  Instantiated for
// <true, true>, <true, false> and <false, false>.  defer != 0: split-K partials (and the fused column sums) stay in g.part / g.colsum
// for a later reduce_segments launch; wt: 1 / 2 forces the 64 / 128 tile; half: gemm_h_kernel
template <bool A_KC, bool B_KC>
void launch_gemm(const GemmArgs& g, hipStream_t s, int defer = 0, int wt = 0, int half = 0);

// out[c] += sum_r X[r][c], in a fixed order
#define COLSUM_CHUNKS 128
void colsum_det(const float* X, int rows, int ld, int ncols, float* out, float* scratch /* [COLSUM_CHUNKS][ncols] */, hipStream_t s);

// Ordered reduction of split-K partials that were left in place by a series of GEMMs (the weight / bias gradients of one
// minibatch): one launch adds every segment's slices, in slice order, to its destination.
#define MAX_SEGS 16
struct Seg { const float* part; float* dst; int nslices, count, N, ldc; };   // partial z at part + z*count; element i -> dst[(i/N)*ldc + i%N]
struct SegList { Seg s[MAX_SEGS]; int first[MAX_SEGS + 1]; int n; float scale; };   // scale: applied to every total (undoes the loss scaling)
void seg_add(SegList& L, const float* part, float* dst, int nslices, int M, int N, int ldc);
void launch_reduce_segments(const SegList& L, hipStream_t s);

// wgrad_skinny_kernel: dW1 / db1 / dW3 / db3 of one network in one K-streaming launch of ceil(R / kc) blocks
struct WgradSkinnyArgs {
  const float *dh1, *x, *dy, *h2;   // [R][256], [R][ldx], [R][Op], [R][256]
  int ldx, Dp, O, Op, R, kc;
  float *pw1, *pb1, *pw3, *pb3;     // slice z: pw1 + z * 256 * Dp, pb1 + z * 256, pw3 + z * O * 256, pb3 + z * O
};
bool fused_skinny_on();   // LHW_WGRAD_FUSED
int wgrad_skinny_chunk(int R);
bool wgrad_skinny_supported(int H, int Dp, int O, int Op);
void launch_wgrad_skinny(const WgradSkinnyArgs& a, hipStream_t s);
// wgrad_wide_kernel: dW2 [256][256] = A^T B and db2 = colsum(A) per k slice, A = dh2, B = h1, both [K][256]
bool wgrad_wide_on();     // LHW_WGRAD_WIDE
bool wgrad_wide_supported(int H);
void launch_wgrad_wide(const float* A, const float* B, int K, int k_chunk, float* part, float* colsum, hipStream_t s);
