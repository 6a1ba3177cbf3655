// batchnorm.hip — K18: batch normalization over NCHW tensors (fp32 or bf16)
// with an optional fused residual add and ReLU, forward and backward.
//
// Contract (the CPU path of ops.batchnorm2d is the plain-torch form of it):
// statistics and all arithmetic are fp32; the variance comes from centred
// values (per-slice mean, then the centred second moment of the slice;
// slices merged with Chan's formula); every output element is rounded once
// to its dtype; no float atomics — every cross-workgroup sum goes through
// a partial buffer combined in fixed index order, so the statistics,
// dgamma, dbeta and everything computed from them are bitwise reproducible.
//
// Kernels:
//   bn_stats_kernel         grid (C, S): block (c, s) reduces planes
//                           [s*P, min(B, (s+1)*P)) of channel c to
//                           (count, mean, M2) in ws[C][S][3]
//   bn_finalize_kernel      merges the S partials in order, writes
//                           save_mean / save_invstd, updates the running
//                           buffers on the stream
//   bn_apply_kernel         y = relu?((x-mean)*(gamma*invstd)+beta (+res))
//   bn_bwd_reduce_kernel    grid (C, S): partial dbeta / dgamma, ws[C][S][2]
//   bn_bwd_finalize_kernel  sums the partials in order
//   bn_bwd_apply_kernel     gx and/or g_residual in one pass
//
// Memory access.  A plane starts at (b*C + c)*HW elements, so its
// alignment depends on HW and on the base pointer.  Every launch picks the
// widest access of V elements (16, 8, 4 or 2 bytes) for which HW % V == 0
// and every pointer is V-element aligned: then no access straddles a plane
// or is misaligned, and there is nothing to peel.  56x56, 28x28 and
// 112x112 planes move 16 bytes per lane in both dtypes; 14x14 bf16 planes
// 8 bytes; 7x7 planes one element.
//
// Reduction order.  The sums must not depend on V (a view with another
// alignment, or the bf16 form of the same values, has to give the same
// bits), so the order is fixed on elements, not on accesses: element e of a
// slice belongs to group e/8, group g to thread g % 256, and the thread
// keeps one accumulator per e % 8.  A thread reads its group as 8/V
// accesses of V elements.  The eight accumulators are added as a fixed
// tree, the 64 lanes by wave shuffles, the 4 waves through LDS.
//
// The access (load_vec / store_vec), the two sums (tree8, block_sum) and
// the dispatch on dtype and width (by_dtype_width) are common.h's.
//
// Bindings are registered from kernels.hip's PYBIND11_MODULE through
// register_batchnorm().

#include "common.h"

#include <pybind11/pybind11.h>

#include <algorithm>
#include <initializer_list>

namespace {

constexpr int GROUP = 8;  // elements per accumulation group

// The slice of block (c, s) = (blockIdx.x, blockIdx.y): nb planes of HW
// elements, plane p at first + p*pstride.
struct Slice {
  int64_t first;     // element offset of the slice's first plane
  int64_t pstride;   // elements between two planes of one channel
  uint32_t nb;       // planes in the slice
};

__device__ __forceinline__ Slice slice_of(int B, int C, int HW, int P) {
  const int b0 = blockIdx.y * P;
  Slice s;
  s.first = ((int64_t)b0 * C + blockIdx.x) * HW;
  s.pstride = (int64_t)C * HW;
  s.nb = (uint32_t)min(P, B - b0);
  return s;
}

// ---------------------------------------------------------------------------
// forward statistics
// ---------------------------------------------------------------------------
template <typename T, int V>
__global__ __launch_bounds__(BLK) void bn_stats_kernel(
    const T* __restrict__ x, float* __restrict__ ws, int B, int C, int HW,
    int P) {
  __shared__ float sh[NWAVE];
  constexpr int NA = GROUP / V;  // accesses per group
  const Slice sl = slice_of(B, C, HW, P);
  const uint32_t hwv = (uint32_t)HW / V;
  const uint32_t nvec = sl.nb * hwv;
  const T* base = x + sl.first;

  float acc[GROUP];
#pragma unroll
  for (int j = 0; j < GROUP; ++j) acc[j] = 0.f;
  for (uint32_t g = threadIdx.x; g * NA < nvec; g += BLK) {
#pragma unroll
    for (int k = 0; k < NA; ++k) {
      const uint32_t q = g * NA + k;
      if (q < nvec) {
        const uint32_t pl = q / hwv, off = q - pl * hwv;
        float f[V];
        load_vec<T, V>(base + pl * sl.pstride + (int64_t)off * V, f);
#pragma unroll
        for (int j = 0; j < V; ++j) acc[k * V + j] += f[j];
      }
    }
  }
  const float cnt = (float)sl.nb * (float)HW;
  const float mean = block_sum(tree8(acc), sh) / cnt;

  // second pass over the slice (L2-resident): centred second moment
#pragma unroll
  for (int j = 0; j < GROUP; ++j) acc[j] = 0.f;
  for (uint32_t g = threadIdx.x; g * NA < nvec; g += BLK) {
#pragma unroll
    for (int k = 0; k < NA; ++k) {
      const uint32_t q = g * NA + k;
      if (q < nvec) {
        const uint32_t pl = q / hwv, off = q - pl * hwv;
        float f[V];
        load_vec<T, V>(base + pl * sl.pstride + (int64_t)off * V, f);
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const float d = f[j] - mean;
          acc[k * V + j] = fmaf(d, d, acc[k * V + j]);
        }
      }
    }
  }
  const float m2 = block_sum(tree8(acc), sh);
  if (threadIdx.x == 0) {
    float* o = ws + ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * 3;
    o[0] = cnt;
    o[1] = mean;
    o[2] = m2;
  }
}

__global__ void bn_finalize_kernel(const float* __restrict__ ws, int C, int S,
                                   float eps, float momentum,
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

// ---------------------------------------------------------------------------
// forward apply (+ residual, + ReLU)
// ---------------------------------------------------------------------------
template <typename T, int V>
__global__ __launch_bounds__(BLK) void bn_apply_kernel(
    const T* __restrict__ x, const T* __restrict__ res, T* __restrict__ y,
    const float* __restrict__ mean, const float* __restrict__ stat,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    float eps, int eval, int relu, uint32_t nvec, uint32_t hwv, uint32_t C) {
  for (uint32_t q = blockIdx.x * BLK + threadIdx.x; q < nvec;
       q += gridDim.x * BLK) {
    const uint32_t c = (q / hwv) % C;
    float mu, inv;
    channel_stats(mean, stat, eps, eval, c, mu, inv);
    const float sc = gamma[c] * inv, be = beta[c];
    float f[V], r[V];
    load_vec<T, V>(x + (int64_t)q * V, f);
    if (res) load_vec<T, V>(res + (int64_t)q * V, r);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      float t = fmaf(f[j] - mu, sc, be);
      if (res) t += r[j];
      if (relu) t = t > 0.f ? t : 0.f;
      f[j] = t;
    }
    store_vec<T, V>(y + (int64_t)q * V, f);
  }
}

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------
template <typename T, int V>
__global__ __launch_bounds__(BLK) void bn_bwd_reduce_kernel(
    const T* __restrict__ x, const T* __restrict__ gy,
    const T* __restrict__ y, const float* __restrict__ mean,
    const float* __restrict__ stat, float eps, int eval,
    float* __restrict__ ws, int B, int C, int HW, int P) {
  __shared__ float sh[NWAVE];
  constexpr int NA = GROUP / V;
  const Slice sl = slice_of(B, C, HW, P);
  const uint32_t hwv = (uint32_t)HW / V;
  const uint32_t nvec = sl.nb * hwv;
  float mu, inv;
  channel_stats(mean, stat, eps, eval, blockIdx.x, mu, inv);

  float db[GROUP], dg[GROUP];
#pragma unroll
  for (int j = 0; j < GROUP; ++j) db[j] = dg[j] = 0.f;
  for (uint32_t g = threadIdx.x; g * NA < nvec; g += BLK) {
#pragma unroll
    for (int k = 0; k < NA; ++k) {
      const uint32_t q = g * NA + k;
      if (q < nvec) {
        const uint32_t pl = q / hwv, off = q - pl * hwv;
        const int64_t at = sl.first + pl * sl.pstride + (int64_t)off * V;
        float fx[V], fg[V], fy[V];
        load_vec<T, V>(x + at, fx);
        load_vec<T, V>(gy + at, fg);
        if (y) load_vec<T, V>(y + at, fy);
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const float gj = (y && !(fy[j] > 0.f)) ? 0.f : fg[j];
          const float xh = (fx[j] - mu) * inv;
          db[k * V + j] += gj;
          dg[k * V + j] = fmaf(gj, xh, dg[k * V + j]);
        }
      }
    }
  }
  const float sdb = block_sum(tree8(db), sh);
  const float sdg = block_sum(tree8(dg), sh);
  if (threadIdx.x == 0) {
    float* o = ws + ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * 2;
    o[0] = sdb;
    o[1] = sdg;
  }
}

__global__ void bn_bwd_finalize_kernel(const float* __restrict__ ws, int C,
                                       int S, float* __restrict__ dgamma,
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

template <typename T, int V>
__global__ __launch_bounds__(BLK) void bn_bwd_apply_kernel(
    const T* __restrict__ x, const T* __restrict__ gy,
    const T* __restrict__ y, const float* __restrict__ mean,
    const float* __restrict__ stat, const float* __restrict__ gamma,
    const float* __restrict__ dgamma, const float* __restrict__ dbeta,
    T* __restrict__ gx, T* __restrict__ gres, float eps, int eval, float n,
    uint32_t nvec, uint32_t hwv, uint32_t C) {
  for (uint32_t q = blockIdx.x * BLK + threadIdx.x; q < nvec;
       q += gridDim.x * BLK) {
    const uint32_t c = (q / hwv) % C;
    const int64_t at = (int64_t)q * V;
    float fg[V], fy[V];
    load_vec<T, V>(gy + at, fg);
    if (y) {
      load_vec<T, V>(y + at, fy);
#pragma unroll
      for (int j = 0; j < V; ++j)
        if (!(fy[j] > 0.f)) fg[j] = 0.f;
    }
    if (gres) store_vec<T, V>(gres + at, fg);
    if (gx) {
      float mu, inv;
      channel_stats(mean, stat, eps, eval, c, mu, inv);
      const float sc = gamma[c] * inv;
      float o[V];
      if (eval) {
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = sc * fg[j];
      } else {
        const float k1 = dbeta[c] / n, k2 = dgamma[c] / n;
        float fx[V];
        load_vec<T, V>(x + at, fx);
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const float xh = (fx[j] - mu) * inv;
          o[j] = sc * ((fg[j] - k1) - xh * k2);
        }
      }
      store_vec<T, V>(gx + at, o);
    }
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
constexpr int64_t MAX_ELEMS = (int64_t)1 << 31;  // 32-bit access indices

void check_dims(int64_t B, int64_t C, int64_t HW) {
  if (B < 1 || C < 1 || HW < 1)
    throw std::invalid_argument("batchnorm2d: B, C and H*W must be >= 1");
  if (B >= MAX_ELEMS || C >= MAX_ELEMS || HW >= MAX_ELEMS ||
      B * C >= MAX_ELEMS || B * C * HW >= MAX_ELEMS)
    throw std::invalid_argument(
        "batchnorm2d: more than 2^31 - 1 elements are not supported");
}

// How many slices the planes of one channel are split into.  Enough blocks
// to fill the chip when channels are few (aim: 8 per CU on 256 CUs), but a
// slice keeps at least 2048 elements (8 per thread), so many channels of
// few pixels are not split to nothing.  Shapes only.
int batchnorm2d_splits(int64_t B, int64_t C, int64_t HW) {
  check_dims(B, C, HW);
  const int64_t want = (2048 + C - 1) / C;
  const int64_t by_size = B * HW / 2048;
  int64_t s = std::min(std::min(B, want), std::min(by_size, (int64_t)1024));
  if (s < 1) s = 1;
  const int64_t per = (B + s - 1) / s;  // planes per slice
  return (int)((B + per - 1) / per);    // no empty slice
}

// widest access (in elements) that is aligned for every plane and pointer
int pick_v(int elem_bytes, int64_t HW, std::initializer_list<uintptr_t> ptrs) {
  for (int v = 16 / elem_bytes; v > 1; v >>= 1) {
    bool ok = HW % v == 0;
    for (uintptr_t p : ptrs) ok = ok && p % (uintptr_t)(v * elem_bytes) == 0;
    if (ok) return v;
  }
  return 1;
}

int planes_per_slice(int64_t B, int64_t C, int64_t HW, int S) {
  if (S != batchnorm2d_splits(B, C, HW))
    throw std::invalid_argument(
        "batchnorm2d: splits must come from batchnorm2d_splits");
  return (int)((B + S - 1) / S);
}

// Training: statistics of x into save_mean / save_invstd (and the running
// buffers, when given), then y.  Eval: y from running_mean / running_var;
// save_mean, save_invstd and ws are not touched and may be 0.
void batchnorm2d_fwd(uintptr_t x, uintptr_t res, uintptr_t y, uintptr_t gamma,
                     uintptr_t beta, uintptr_t run_mean, uintptr_t run_var,
                     uintptr_t save_mean, uintptr_t save_invstd, uintptr_t ws,
                     int splits, int64_t B, int64_t C, int64_t HW,
                     bool training, double momentum, double eps, bool relu,
                     bool is_bf16, uintptr_t stream) {
  check_dims(B, C, HW);
  if (!training && (!run_mean || !run_var))
    throw std::invalid_argument(
        "batchnorm2d: eval mode needs the running statistics");
  if (training && (!save_mean || !save_invstd || !ws))
    throw std::invalid_argument(
        "batchnorm2d: training needs save_mean, save_invstd and a workspace");
  if (training && B * HW < 2)
    throw std::invalid_argument(
        "batchnorm2d: training needs more than one value per channel");
  if ((run_mean == 0) != (run_var == 0))
    throw std::invalid_argument(
        "batchnorm2d: running_mean and running_var come together");
  const int es = is_bf16 ? 2 : 4;
  if (training) {
    const int P = planes_per_slice(B, C, HW, splits);
    by_dtype_width(is_bf16, pick_v(es, HW, {x}), [&](auto* t, auto v) {
      using T = elem_t<decltype(t)>;
      hipLaunchKernelGGL((bn_stats_kernel<T, v()>), dim3(C, splits), dim3(BLK),
                         0, S(stream), (const T*)x, (float*)ws, (int)B, (int)C,
                         (int)HW, P);
    });
    hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + 63) / 64), dim3(64), 0,
                       S(stream), (const float*)ws, (int)C, splits,
                       (float)eps, (float)momentum, (float*)save_mean,
                       (float*)save_invstd, (float*)run_mean,
                       (float*)run_var);
  }
  const uintptr_t mean = training ? save_mean : run_mean;
  const uintptr_t stat = training ? save_invstd : run_var;
  by_dtype_width(is_bf16, pick_v(es, HW, {x, res, y}), [&](auto* t, auto v) {
    using T = elem_t<decltype(t)>;
    const uint32_t hwv = (uint32_t)HW / v();
    const uint32_t nvec = (uint32_t)B * (uint32_t)C * hwv;
    hipLaunchKernelGGL((bn_apply_kernel<T, v()>), dim3(grid_for(nvec, BLK)),
                       dim3(BLK), 0, S(stream), (const T*)x, (const T*)res,
                       (T*)y, (const float*)mean, (const float*)stat,
                       (const float*)gamma, (const float*)beta, (float)eps,
                       (int)!training, (int)relu, nvec, hwv, (uint32_t)C);
  });
  HIP_CHECK(hipGetLastError());
}

// dgamma and dbeta are always written (the training gx needs them); gx and
// gres are written when non-zero.  mean/stat are the saved statistics in
// training and running_mean / running_var in eval; y is the forward output
// when ReLU was fused, else 0.
void batchnorm2d_bwd(uintptr_t x, uintptr_t gy, uintptr_t y, uintptr_t gamma,
                     uintptr_t mean, uintptr_t stat, uintptr_t dgamma,
                     uintptr_t dbeta, uintptr_t gx, uintptr_t gres,
                     uintptr_t ws, int splits, int64_t B, int64_t C,
                     int64_t HW, bool training, double eps, bool is_bf16,
                     uintptr_t stream) {
  check_dims(B, C, HW);
  if (!x || !gy || !mean || !stat || !gamma || !dgamma || !dbeta || !ws)
    throw std::invalid_argument("batchnorm2d_bwd: null tensor");
  const int es = is_bf16 ? 2 : 4;
  const int P = planes_per_slice(B, C, HW, splits);
  const int eval = !training;
  by_dtype_width(is_bf16, pick_v(es, HW, {x, gy, y}), [&](auto* t, auto v) {
    using T = elem_t<decltype(t)>;
    hipLaunchKernelGGL((bn_bwd_reduce_kernel<T, v()>), dim3(C, splits),
                       dim3(BLK), 0, S(stream), (const T*)x, (const T*)gy,
                       (const T*)y, (const float*)mean, (const float*)stat,
                       (float)eps, eval, (float*)ws, (int)B, (int)C, (int)HW,
                       P);
  });
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((C + 63) / 64), dim3(64), 0,
                     S(stream), (const float*)ws, (int)C, splits,
                     (float*)dgamma, (float*)dbeta);
  if (gx || gres)
    by_dtype_width(
        is_bf16, pick_v(es, HW, {x, gy, y, gx, gres}), [&](auto* t, auto v) {
          using T = elem_t<decltype(t)>;
          const uint32_t hwv = (uint32_t)HW / v();
          const uint32_t nvec = (uint32_t)B * (uint32_t)C * hwv;
          hipLaunchKernelGGL(
              (bn_bwd_apply_kernel<T, v()>), dim3(grid_for(nvec, BLK)),
              dim3(BLK), 0, S(stream), (const T*)x, (const T*)gy, (const T*)y,
              (const float*)mean, (const float*)stat, (const float*)gamma,
              (const float*)dgamma, (const float*)dbeta, (T*)gx, (T*)gres,
              (float)eps, eval, (float)B * (float)HW, nvec, hwv, (uint32_t)C);
        });
  HIP_CHECK(hipGetLastError());
}

}  // namespace

void register_batchnorm(pybind11::module_& m) {
  m.def("batchnorm2d_splits", &batchnorm2d_splits);
  m.def("batchnorm2d_fwd", &batchnorm2d_fwd);
  m.def("batchnorm2d_bwd", &batchnorm2d_bwd);
}
