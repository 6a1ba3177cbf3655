// pointwise.hip — K3-K6: the pointwise and pooling ops of the training
// path, for fp32 and bf16 activations: fused 2x2 maxpool+ReLU, ReLU,
// elementwise and channel dropout, the fp32 -> bf16 cast and the
// device-seed advance.
//
// pool, dropout and dropout2d are one kernel template each, instantiated
// for float and bf16_t (raw bits, common.h).  Elements are read with
// to_f() and written with from_f(), so both dtypes run the same index
// arithmetic, the same RNG expression and the same mask writes; the only
// per-type code is the pool's pair access (load_pair / store_pair).
// Bindings take the dtype as a `bool bf16` before the stream and dispatch
// on it with by_dtype; that, and the aligned vector access the bf16 pair
// and the cast use (Vec, load_vec, store_vec), are common.h's.
//
// Grid-stride loops, 256-thread blocks, grids capped by grid_for().
// Bindings are registered from kernels.hip's PYBIND11_MODULE through
// register_pointwise().

#include "common.h"

#include <pybind11/pybind11.h>

namespace {

// ===========================================================================
// K3+K4 — fused 2x2/stride-2 maxpool + ReLU (train_dist.py:65-66).
// Forward stores the winning slot (0..3) in bits 0-1 of idx and "ReLU
// clipped" in bit 2; the first maximum wins a tie.  Max and ReLU only
// select, so the output carries the selected input's bits in either dtype.
// The backward writes all four window slots (pool windows are disjoint),
// so gx needs no pre-zeroing where H and W are even.
//
// Two horizontally adjacent elements are a pair.  fp32: two scalar
// accesses, any H and W (floor semantics), any alignment.  bf16: one
// 4-byte access; H and W are even (checked by the launcher) and the base
// is 4-byte aligned, so every pair is.
// ===========================================================================
template <typename T>
struct Pair {
  T a, b;
};

__device__ __forceinline__ Pair<float> load_pair(const float* p) {
  return {p[0], p[1]};
}
__device__ __forceinline__ Pair<bf16_t> load_pair(const bf16_t* p) {
  Vec<bf16_t, 2> u;
  u.raw = *reinterpret_cast<const uint32_t*>(p);
  return {u.e[0], u.e[1]};
}
__device__ __forceinline__ void store_pair(float* p, Pair<float> v) {
  p[0] = v.a;
  p[1] = v.b;
}
__device__ __forceinline__ void store_pair(bf16_t* p, Pair<bf16_t> v) {
  Vec<bf16_t, 2> u;
  u.e[0] = v.a;
  u.e[1] = v.b;
  *reinterpret_cast<uint32_t*>(p) = u.raw;
}

template <typename T>
__global__ void maxpool2d_relu_fwd_kernel(const T* __restrict__ x,
                                          T* __restrict__ out,
                                          int* __restrict__ idx,
                                          int64_t planes, int H, int W) {
  const int OH = H / 2, OW = W / 2;
  const int64_t n = planes * OH * OW;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = i / (OH * OW);
    const int oh = (int)((i / OW) % OH);
    const int ow = (int)(i % OW);
    const T* xp = x + p * H * W + (int64_t)(oh * 2) * W + ow * 2;
    const Pair<T> top = load_pair(xp), bot = load_pair(xp + W);
    int am = 0;
    T mb = top.a;
    float m = to_f(top.a);
    if (to_f(top.b) > m) { m = to_f(top.b); mb = top.b; am = 1; }
    if (to_f(bot.a) > m) { m = to_f(bot.a); mb = bot.a; am = 2; }
    if (to_f(bot.b) > m) { m = to_f(bot.b); mb = bot.b; am = 3; }
    out[i] = m > 0.f ? mb : T(0);
    idx[i] = m > 0.f ? am : (am | 4);
  }
}

template <typename T>
__global__ void maxpool2d_relu_bwd_kernel(const T* __restrict__ gy,
                                          const int* __restrict__ idx,
                                          T* __restrict__ gx,
                                          int64_t planes, int H, int W) {
  const int OH = H / 2, OW = W / 2;
  const int64_t n = planes * OH * OW;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = i / (OH * OW);
    const int oh = (int)((i / OW) % OH);
    const int ow = (int)(i % OW);
    T* gp = gx + p * H * W + (int64_t)(oh * 2) * W + ow * 2;
    const int v = idx[i];
    const int am = v & 3;
    const T g = (v & 4) ? T(0) : gy[i];
    store_pair(gp, Pair<T>{am == 0 ? g : T(0), am == 1 ? g : T(0)});
    store_pair(gp + W, Pair<T>{am == 2 ? g : T(0), am == 3 ? g : T(0)});
  }
}

// ===========================================================================
// K4 — standalone ReLU (fp32 only, float4-vectorized)
// ===========================================================================
__global__ __launch_bounds__(BLK) void relu_fwd_kernel(
    const float* __restrict__ x, float* __restrict__ out, int64_t n) {
  vec_sweep<float>(n, [=](int64_t i, auto width) {
    constexpr int V = decltype(width)::value;
    float v[V];
    load_vec<float, V>(x + i, v);
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = v[j] > 0.f ? v[j] : 0.f;
    store_vec<float, V>(out + i, v);
  });
}

__global__ void relu_bwd_kernel(const float* __restrict__ gy,
                                const float* __restrict__ out,
                                float* __restrict__ gx, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    gx[i] = out[i] > 0.f ? gy[i] : 0.f;
}

// ===========================================================================
// K5/K6 — dropout.  Counter-based hash RNG (mix32 in common.h) of
// (seed, index): stateless, reproducible from the device seed, no
// RNG-state tensor.  The index is the element for dropout and the
// (batch, channel) plane for the channelwise variant (Dropout2d,
// train_dist.py:60); it does not depend on the dtype, so equal (seed, p)
// gives equal masks in fp32 and bf16.  Kept values are x * scale in fp32,
// rounded once to the element type.
// ===========================================================================
// device-side seed bump: lets dropout RNG advance across hipGraph
// replays (the seed lives in device memory; one tiny kernel increments
// it before each dropout draw, stream-ordered).
__global__ void bump_seed_kernel(unsigned long long* s) {
  if (threadIdx.x == 0 && blockIdx.x == 0)
    *s += SEED_INC;
}

template <typename T>
__global__ void dropout_fwd_kernel(const T* __restrict__ x,
                                   T* __restrict__ out,
                                   uint8_t* __restrict__ mask, int64_t n,
                                   float p, float scale,
                                   const unsigned long long* __restrict__ sp) {
  const uint32_t thresh = (uint32_t)(p * 4294967296.0);
  const uint64_t seed = sp[0];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t r = mix32(seed, (uint64_t)i) << 16 |
                 (mix32(seed ^ 0xabcd, i) & 0xffff);
    uint8_t keep = r >= thresh;
    mask[i] = keep;
    from_f(keep ? to_f(x[i]) * scale : 0.f, out[i]);
  }
}

template <typename T>
__global__ void dropout_bwd_kernel(const T* __restrict__ gy,
                                   const uint8_t* __restrict__ mask,
                                   T* __restrict__ gx, int64_t n,
                                   float scale) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    from_f(mask[i] ? to_f(gy[i]) * scale : 0.f, gx[i]);
}

template <typename T>
__global__ void dropout2d_fwd_kernel(const T* __restrict__ x,
                                     T* __restrict__ out,
                                     uint8_t* __restrict__ mask,
                                     int64_t planes, int64_t hw, float p,
                                     float scale,
                                     const unsigned long long* __restrict__ sp) {
  const uint32_t thresh = (uint32_t)(p * 4294967296.0);
  const uint64_t seed = sp[0];
  const int64_t n = planes * hw;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t pl = i / hw;
    uint32_t r = mix32(seed, (uint64_t)pl) << 16 |
                 (mix32(seed ^ 0xabcd, pl) & 0xffff);
    uint8_t keep = r >= thresh;
    if (i % hw == 0) mask[pl] = keep;
    from_f(keep ? to_f(x[i]) * scale : 0.f, out[i]);
  }
}

template <typename T>
__global__ void dropout2d_bwd_kernel(const T* __restrict__ gy,
                                     const uint8_t* __restrict__ mask,
                                     T* __restrict__ gx, int64_t planes,
                                     int64_t hw, float scale) {
  const int64_t n = planes * hw;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    from_f(mask[i / hw] ? to_f(gy[i]) * scale : 0.f, gx[i]);
}

// ===========================================================================
// cast fp32 -> bf16 (RNE): 8 elements per thread where both pointers are
// 16-byte aligned, one element per thread for the tail or otherwise
// ===========================================================================
__global__ void cast_f32_to_bf16_kernel(const float* __restrict__ src,
                                        bf16_t* __restrict__ dst, int64_t n,
                                        int64_t nvec) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nth = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = tid; i < nvec; i += nth) {
    float f[8];
    load_vec<float, 8>(src + 8 * i, f);
    store_vec<bf16_t, 8>(dst + 8 * i, f);
  }
  for (int64_t i = nvec * 8 + tid; i < n; i += nth) dst[i] = f2bf(src[i]);
}

// ===========================================================================
// host launchers
// ===========================================================================
// planes * (H/2) * (W/2); the bf16 kernels need whole 4-byte pairs
int64_t pool_outputs(int B, int C, int H, int W, bool bf16) {
  if (bf16 && (H < 2 || W < 2 || (H & 1) || (W & 1)))
    throw std::invalid_argument(
        "maxpool2d_relu (bf16): H and W must be even and >= 2");
  return (int64_t)B * C * (H / 2) * (W / 2);
}

void maxpool2d_relu_fwd(uintptr_t x, uintptr_t out, uintptr_t idx, int B,
                        int C, int H, int W, bool bf16, uintptr_t stream) {
  const int64_t n = pool_outputs(B, C, H, W, bf16);
  if (n <= 0) return;
  by_dtype(bf16, [&](auto* t) {
    using T = elem_t<decltype(t)>;
    hipLaunchKernelGGL(maxpool2d_relu_fwd_kernel<T>, dim3(grid_for(n, BLK)),
                       dim3(BLK), 0, S(stream), (const T*)x, (T*)out,
                       (int*)idx, (int64_t)B * C, H, W);
  });
}

void maxpool2d_relu_bwd(uintptr_t gy, uintptr_t idx, uintptr_t gx, int B,
                        int C, int H, int W, bool bf16, uintptr_t stream) {
  const int64_t n = pool_outputs(B, C, H, W, bf16);
  if (n <= 0) return;
  by_dtype(bf16, [&](auto* t) {
    using T = elem_t<decltype(t)>;
    hipLaunchKernelGGL(maxpool2d_relu_bwd_kernel<T>, dim3(grid_for(n, BLK)),
                       dim3(BLK), 0, S(stream), (const T*)gy,
                       (const int*)idx, (T*)gx, (int64_t)B * C, H, W);
  });
}

void relu_fwd(uintptr_t x, uintptr_t out, int64_t n, uintptr_t stream) {
  hipLaunchKernelGGL(relu_fwd_kernel, dim3(grid_for(n, BLK, 4)), dim3(BLK),
                     0, S(stream), (const float*)x, (float*)out, n);
}

void relu_bwd(uintptr_t gy, uintptr_t out, uintptr_t gx, int64_t n,
              uintptr_t stream) {
  hipLaunchKernelGGL(relu_bwd_kernel, dim3(grid_for(n, BLK)), dim3(BLK), 0,
                     S(stream), (const float*)gy, (const float*)out,
                     (float*)gx, n);
}

// The forward scales by 1/(1-p) evaluated in fp32; the backward takes the
// caller's double scale rounded to fp32.  One seed bump per forward call.
void dropout_fwd(uintptr_t x, uintptr_t out, uintptr_t mask, int64_t n,
                 double p, uintptr_t seed_dev, bool bf16, uintptr_t stream) {
  const float scale = 1.f / (1.f - (float)p);
  launch_bump_seed(seed_dev, S(stream));
  by_dtype(bf16, [&](auto* t) {
    using T = elem_t<decltype(t)>;
    hipLaunchKernelGGL(dropout_fwd_kernel<T>, dim3(grid_for(n, BLK)),
                       dim3(BLK), 0, S(stream), (const T*)x, (T*)out,
                       (uint8_t*)mask, n, (float)p, scale,
                       (const unsigned long long*)seed_dev);
  });
}

void dropout_bwd(uintptr_t gy, uintptr_t mask, uintptr_t gx, int64_t n,
                 double scale, bool bf16, uintptr_t stream) {
  by_dtype(bf16, [&](auto* t) {
    using T = elem_t<decltype(t)>;
    hipLaunchKernelGGL(dropout_bwd_kernel<T>, dim3(grid_for(n, BLK)),
                       dim3(BLK), 0, S(stream), (const T*)gy,
                       (const uint8_t*)mask, (T*)gx, n, (float)scale);
  });
}

void dropout2d_fwd(uintptr_t x, uintptr_t out, uintptr_t mask,
                   int64_t planes, int64_t hw, double p, uintptr_t seed_dev,
                   bool bf16, uintptr_t stream) {
  const float scale = 1.f / (1.f - (float)p);
  launch_bump_seed(seed_dev, S(stream));
  by_dtype(bf16, [&](auto* t) {
    using T = elem_t<decltype(t)>;
    hipLaunchKernelGGL(dropout2d_fwd_kernel<T>,
                       dim3(grid_for(planes * hw, BLK)), dim3(BLK), 0,
                       S(stream), (const T*)x, (T*)out, (uint8_t*)mask,
                       planes, hw, (float)p, scale,
                       (const unsigned long long*)seed_dev);
  });
}

void dropout2d_bwd(uintptr_t gy, uintptr_t mask, uintptr_t gx,
                   int64_t planes, int64_t hw, double scale, bool bf16,
                   uintptr_t stream) {
  by_dtype(bf16, [&](auto* t) {
    using T = elem_t<decltype(t)>;
    hipLaunchKernelGGL(dropout2d_bwd_kernel<T>,
                       dim3(grid_for(planes * hw, BLK)), dim3(BLK), 0,
                       S(stream), (const T*)gy, (const uint8_t*)mask,
                       (T*)gx, planes, hw, (float)scale);
  });
}

void cast_f32_to_bf16(uintptr_t src, uintptr_t dst, int64_t n,
                      uintptr_t stream) {
  if (n <= 0) return;
  const int64_t nvec = (src % 16 == 0 && dst % 16 == 0) ? n / 8 : 0;
  hipLaunchKernelGGL(cast_f32_to_bf16_kernel,
                     dim3(grid_for((n + 7) / 8, BLK)), dim3(BLK), 0,
                     S(stream), (const float*)src, (bf16_t*)dst, n, nvec);
}

}  // namespace

void launch_bump_seed(uintptr_t seed_ptr, hipStream_t stream) {
  hipLaunchKernelGGL(bump_seed_kernel, dim3(1), dim3(64), 0, stream,
                     (unsigned long long*)seed_ptr);
}

void register_pointwise(pybind11::module_& m) {
  m.def("maxpool2d_relu_fwd", &maxpool2d_relu_fwd);
  m.def("maxpool2d_relu_bwd", &maxpool2d_relu_bwd);
  m.def("relu_fwd", &relu_fwd);
  m.def("relu_bwd", &relu_bwd);
  m.def("dropout_fwd", &dropout_fwd);
  m.def("dropout_bwd", &dropout_bwd);
  m.def("dropout2d_fwd", &dropout2d_fwd);
  m.def("dropout2d_bwd", &dropout2d_bwd);
  m.def("cast_f32_to_bf16", &cast_f32_to_bf16);
}
