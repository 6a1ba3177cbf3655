// bn_shared.h — what batchnorm.hip (NCHW) and batchnorm_nhwc.hip
// (channels-last) share: the two finalize kernels, which merge the partial
// buffers ws[C][S][3] / ws[C][S][2] in index order whatever kernel filled
// them, the per-channel (mean, invstd) pick and the size guard.  One
// definition each, so the two layouts cannot drift apart.
#pragma once

#include "common.h"

static __global__ void bn_finalize_kernel(const float* __restrict__ ws, int C,
                                          int S, float eps, float momentum,
                                          float* __restrict__ save_mean,
                                          float* __restrict__ save_invstd,
                                          float* __restrict__ run_mean,
                                          float* __restrict__ run_var) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float* p = ws + (int64_t)c * S * 3;
  float n = p[0], mean = p[1], m2 = p[2];
  for (int s = 1; s < S; ++s) {  // Chan's merge, in index order
    const float nb = p[3 * s], mb = p[3 * s + 1], m2b = p[3 * s + 2];
    const float nab = n + nb, delta = mb - mean;
    mean += delta * (nb / nab);
    m2 += m2b + delta * delta * (n * (nb / nab));
    n = nab;
  }
  const float var = m2 / n;
  save_mean[c] = mean;
  save_invstd[c] = 1.f / sqrtf(var + eps);
  if (run_mean) {
    const float keep = 1.f - momentum;
    run_mean[c] = keep * run_mean[c] + momentum * mean;
    run_var[c] = keep * run_var[c] + momentum * (var * (n / (n - 1.f)));
  }
}

// per-channel (mean, invstd): the saved statistics in training, the running
// ones in eval (stat = running_var there)
__device__ __forceinline__ void channel_stats(const float* mean,
                                              const float* stat, float eps,
                                              int eval, uint32_t c, float& mu,
                                              float& inv) {
  mu = mean[c];
  inv = eval ? 1.f / sqrtf(stat[c] + eps) : stat[c];
}

static __global__ void bn_bwd_finalize_kernel(const float* __restrict__ ws,
                                              int C, int S,
                                              float* __restrict__ dgamma,
                                              float* __restrict__ dbeta) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float* p = ws + (int64_t)c * S * 2;
  float db = p[0], dg = p[1];
  for (int s = 1; s < S; ++s) {
    db += p[2 * s];
    dg += p[2 * s + 1];
  }
  dbeta[c] = db;
  dgamma[c] = dg;
}

constexpr int64_t BN_MAX_ELEMS = (int64_t)1 << 31;  // 32-bit access indices

inline void check_dims(int64_t B, int64_t C, int64_t HW) {
  if (B < 1 || C < 1 || HW < 1)
    throw std::invalid_argument("batchnorm2d: B, C and H*W must be >= 1");
  if (B >= BN_MAX_ELEMS || C >= BN_MAX_ELEMS || HW >= BN_MAX_ELEMS ||
      B * C >= BN_MAX_ELEMS || B * C * HW >= BN_MAX_ELEMS)
    throw std::invalid_argument(
        "batchnorm2d: more than 2^31 - 1 elements are not supported");
}
