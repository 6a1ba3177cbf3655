// K16 — bf16 mixed-precision linear on the CDNA4 matrix cores (gfx950).
//
// Numeric contract (ops.linear_bf16): every GEMM operand is bf16, products
// accumulate in fp32 on v_mfma_f32_16x16x32_bf16, and each result is rounded
// ONCE (RNE) from the fp32 accumulator to its output dtype.  fp32 operands
// (master weights, the first layer's input, an fp32 upstream gradient) are
// rounded to bf16 by cast_f32_to_bf16 (pointwise.hip) first.
//
// One GEMM (gemm_bf16.h, shared with the bf16 convolution in
// conv_bf16.hip) serves all three products.  It computes
//     C[m][n] = sum_k A(m,k) * B(n,k)
// from two LDS tiles As[m][k], Bs[n][k] (both K-contiguous, so MFMA
// fragments are one 16-byte LDS read each); what differs per product is the
// global->LDS loader:
//     forward   out = x  · wᵀ   A = x  plain        B = w plain
//     gx            = gy'· w    A = gy plain+mask   B = w transposed on write
//     gw            = gy'ᵀ· x   A = gy transposed+mask, B = x transposed
// gy' = gy where the saved (ReLU-fused) output is > 0; the mask is applied
// while gy is staged.  gw is fp32 and split over the batch through a
// partial buffer that a second kernel sums in split order: no float
// atomics, bitwise reproducible.  gb rides along in the gw kernel.
//
// Bindings are registered from kernels.hip's PYBIND11_MODULE through
// register_linear_bf16().

#include "gemm_bf16.h"

#include <pybind11/pybind11.h>

namespace {

// ---------------------------------------------------------------------------
// the GEMM kernel: gemm_bf16_block (gemm_bf16.h) behind the plain loaders,
// row-major output.  grid = (m tiles, n tiles, splits).
// ---------------------------------------------------------------------------
template <bool TA, bool TB, typename OutT>
__global__ __launch_bounds__(BLK) void gemm_bf16_kernel(
    Operand A, Operand B, int Kred, int kchunk, OutT* __restrict__ C,
    const float* __restrict__ bias, int relu, float* __restrict__ colsum) {
  const int M = A.rows, N = B.rows;
  gemm_bf16_block<TA, TB>(PlainLoader<TA>{A}, PlainLoader<TB>{B}, M, N, Kred,
                          kchunk, bias, relu, colsum,
                          RowMajorOut<OutT>{C, M, N});
}

// ---------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------
static void check_dims(int B, int K, int N) {
  if (B < 1 || K < 1 || N < 1)
    throw std::invalid_argument("linear_bf16: B, K, N must be >= 1");
}

// out[B,N] = x[B,K] · w[N,K]ᵀ (+ bias) (ReLU); x, w bf16
void linear_bf16_fwd(uintptr_t x, uintptr_t w, uintptr_t bias, uintptr_t out,
                     int B, int K, int N, bool relu, bool out_f32,
                     uintptr_t stream) {
  check_dims(B, K, N);
  const Operand a = operand(x, K, B), b = operand(w, K, N);
  const dim3 grid(cdiv(B, BM), cdiv(N, BN), 1);
  if (out_f32)
    hipLaunchKernelGGL((gemm_bf16_kernel<false, false, float>), grid,
                       dim3(BLK), 0, S(stream), a, b, K, K, (float*)out,
                       (const float*)bias, (int)relu, (float*)nullptr);
  else
    hipLaunchKernelGGL((gemm_bf16_kernel<false, false, bf16_t>), grid,
                       dim3(BLK), 0, S(stream), a, b, K, K, (bf16_t*)out,
                       (const float*)bias, (int)relu, (float*)nullptr);
}

// gx[B,K] = gy'[B,N] · w[N,K]; mask (the saved output, 0 = none) has gy's
// layout and is bf16 or fp32
void linear_bf16_bwd_x(uintptr_t gy, uintptr_t w, uintptr_t mask,
                       bool mask_f32, uintptr_t gx, int B, int K, int N,
                       bool out_f32, uintptr_t stream) {
  check_dims(B, K, N);
  const Operand a = operand(gy, N, B, mask, mask_f32);
  const Operand b = operand(w, K, K);  // B(n=k_col, k=n) = w[n*K + k_col]
  const dim3 grid(cdiv(B, BM), cdiv(K, BN), 1);
  if (out_f32)
    hipLaunchKernelGGL((gemm_bf16_kernel<false, true, float>), grid, dim3(BLK),
                       0, S(stream), a, b, N, N, (float*)gx,
                       (const float*)nullptr, 0, (float*)nullptr);
  else
    hipLaunchKernelGGL((gemm_bf16_kernel<false, true, bf16_t>), grid,
                       dim3(BLK), 0, S(stream), a, b, N, N, (bf16_t*)gx,
                       (const float*)nullptr, 0, (float*)nullptr);
}

// How many batch splits the weight gradient uses: enough blocks to cover
// the 256 CUs twice, each split at least two LDS tiles deep.
int linear_bf16_gw_splits(int B, int K, int N) {
  check_dims(B, K, N);
  return gw_split_count(B, N, K);
}

// gw[N,K] = gy'ᵀ · x (fp32), gb[N] = sum_b gy' (fp32, 0 = skip).
// part: fp32 workspace of splits*(N*K + N) floats (unused when splits == 1).
void linear_bf16_bwd_w(uintptr_t gy, uintptr_t x, uintptr_t mask,
                       bool mask_f32, uintptr_t gw, uintptr_t gb,
                       uintptr_t part, int splits, int B, int K, int N,
                       uintptr_t stream) {
  check_dims(B, K, N);
  if (splits != linear_bf16_gw_splits(B, K, N))
    throw std::invalid_argument("linear_bf16_bwd_w: wrong split count");
  const Operand a = operand(gy, N, N, mask, mask_f32);  // A(n, b)
  const Operand b = operand(x, K, K);                   // B(k, b)
  const int kchunk = cdiv(cdiv(B, splits), BK) * BK;
  const dim3 grid(cdiv(N, BM), cdiv(K, BN), splits);
  const int64_t n_gw = (int64_t)N * K;
  float* c = (float*)gw;
  float* cs = (float*)gb;
  if (splits > 1) {
    if (!part) throw std::invalid_argument("linear_bf16_bwd_w: no workspace");
    c = (float*)part;
    cs = gb ? c + (int64_t)splits * n_gw : nullptr;
  }
  hipLaunchKernelGGL((gemm_bf16_kernel<true, true, float>), grid, dim3(BLK), 0,
                     S(stream), a, b, B, kchunk, c, (const float*)nullptr, 0,
                     cs);
  if (splits > 1)
    hipLaunchKernelGGL(gw_combine_kernel, dim3(grid_for(n_gw, BLK)),
                       dim3(BLK), 0, S(stream), (const float*)c, (float*)gw,
                       n_gw, (const float*)cs, (float*)gb, N, splits);
}

}  // namespace

void register_linear_bf16(pybind11::module_& m) {
  m.def("linear_bf16_fwd", &linear_bf16_fwd);
  m.def("linear_bf16_bwd_x", &linear_bf16_bwd_x);
  m.def("linear_bf16_gw_splits", &linear_bf16_gw_splits);
  m.def("linear_bf16_bwd_w", &linear_bf16_bwd_w);
}
