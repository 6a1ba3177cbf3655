// common.h — what the HIP translation units of _kernels.so share:
// error check, stream cast, grid sizing, the dropout RNG and the
// device-seed advance.  One definition each, so the fp32, bf16 and
// fused-Net dropout paths cannot drift apart.
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

constexpr int BLK = 256;  // threads per block of the elementwise kernels

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
// kernel; defined in kernels.hip)
void launch_bump_seed(uintptr_t seed_ptr, hipStream_t stream);
