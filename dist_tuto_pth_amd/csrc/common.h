// common.h — what the HIP translation units of _kernels.so share:
// error check, stream cast, grid sizing, the bf16 element type and its
// conversions, the dropout RNG and the device-seed advance.  One
// definition each, so the fp32, bf16 and fused-Net paths cannot drift
// apart.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>

#define HIP_CHECK(cmd)                                                        \
  do {                                                                        \
    hipError_t e_ = (cmd);                                                    \
    if (e_ != hipSuccess)                                                     \
      throw std::runtime_error(std::string("HIP error: ") +                   \
                               hipGetErrorString(e_) + " @ " #cmd);           \
  } while (0)

constexpr int BLK = 256;  // threads per block (4 waves): the elementwise
                          // kernels, the bf16 GEMM tile and batchnorm

static inline hipStream_t S(uintptr_t s) {
  return reinterpret_cast<hipStream_t>(s);
}

static inline int grid_for(int64_t work, int block, int per_thread = 1) {
  int64_t g = (work + (int64_t)block * per_thread - 1) /
              ((int64_t)block * per_thread);
  if (g > 4096) g = 4096;  // grid-stride beyond (G11: ~8 blocks/CU cap)
  if (g < 1) g = 1;
  return (int)g;
}

// Elements are fp32 or bf16; bf16 travels as raw bits and all arithmetic
// goes through fp32.  to_f / from_f are the typed load and store
// conversions the templated kernels use.
using bf16_t = uint16_t;

__device__ __forceinline__ float to_f(float v) { return v; }
__device__ __forceinline__ float to_f(bf16_t v) {
  return __uint_as_float((uint32_t)v << 16);
}

// fp32 -> bf16, round-to-nearest-even, NaN kept quiet (torch's rule)
__device__ __forceinline__ bf16_t f2bf(float f) {
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (bf16_t)0x7fc0;
  u += 0x7fffu + ((u >> 16) & 1u);
  return (bf16_t)(u >> 16);
}

__device__ __forceinline__ void from_f(float v, float& o) { o = v; }
__device__ __forceinline__ void from_f(float v, bf16_t& o) { o = f2bf(v); }

// Dropout RNG: counter-based hash (splitmix64 finalizer) of
// (seed, index) — stateless, reproducible from the device seed.
__device__ inline uint32_t mix32(uint64_t seed, uint64_t idx) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * (idx + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)((z ^ (z >> 31)) >> 16);
}

// what one advance adds to the device-side dropout seed
constexpr unsigned long long SEED_INC = 0x9E3779B97F4A7C15ull;

// advance the device seed by SEED_INC, stream-ordered (one tiny
// kernel; defined in pointwise.hip)
void launch_bump_seed(uintptr_t seed_ptr, hipStream_t stream);
