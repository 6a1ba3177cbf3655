// common.h — what the HIP translation units of _kernels.so share:
// error check, stream cast, grid sizing, the bf16 element type and its
// conversions, the aligned vector access (Raw, Vec, load_vec, store_vec),
// the vector-then-tail sweep built on it (vec_sweep),
// the fixed-order sums (tree8, block_sum), the dispatch on dtype and access
// width (by_dtype, by_dtype_width), the dropout RNG and the device-seed
// advance.  One definition each, so the fp32, bf16 and fused-Net paths
// cannot drift apart.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>
#include <type_traits>

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

// V elements in one aligned access, converted through fp32.  The caller
// guarantees that p is aligned to the access: sizeof(T)*V bytes, 16 for the
// 32-byte one, which is two 16-byte accesses.
template <int BYTES> struct Raw;
template <> struct Raw<2> { using type = uint16_t; };
template <> struct Raw<4> { using type = uint32_t; };
template <> struct Raw<8> { using type = uint2; };
template <> struct Raw<16> { using type = uint4; };
template <> struct Raw<32> { struct type { uint4 lo, hi; }; };

template <typename T, int V>
union Vec {
  typename Raw<sizeof(T) * V>::type raw;
  T e[V];
};

template <typename T, int V>
__device__ __forceinline__ void load_vec(const T* p, float (&f)[V]) {
  Vec<T, V> u;
  u.raw = *reinterpret_cast<const typename Raw<sizeof(T) * V>::type*>(p);
#pragma unroll
  for (int j = 0; j < V; ++j) f[j] = to_f(u.e[j]);
}

template <typename T, int V>
__device__ __forceinline__ void store_vec(T* p, const float (&f)[V]) {
  Vec<T, V> u;
#pragma unroll
  for (int j = 0; j < V; ++j) from_f(f[j], u.e[j]);
  *reinterpret_cast<typename Raw<sizeof(T) * V>::type*>(p) = u.raw;
}

// Grid-stride sweep over n elements of T, 16 bytes at a time and then a
// scalar tail: calls f(i, integral_constant<int, V>) for the V elements
// from i, with V = 16 / sizeof(T) in the body and V = 1 in the tail.  The
// caller guarantees that whatever f reads or writes V-wide at i is aligned,
// and launches BLK threads per block (blockDim.x read in a device function
// costs a dependent load at the start of the kernel).
template <typename T, class F>
__device__ __forceinline__ void vec_sweep(int64_t n, F&& f) {
  constexpr int V = 16 / sizeof(T);
  const int64_t tid = (int64_t)blockIdx.x * BLK + threadIdx.x;
  const int64_t nth = (int64_t)gridDim.x * BLK;
  const int64_t nvec = n / V;
  for (int64_t i = tid; i < nvec; i += nth)
    f(i * V, std::integral_constant<int, V>{});
  for (int64_t i = nvec * V + tid; i < n; i += nth)
    f(i, std::integral_constant<int, 1>{});
}

// Fixed-order sums: the bits of every reduction built on them depend on
// nothing but these two trees.
__device__ __forceinline__ float tree8(const float (&a)[8]) {
  return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
}

constexpr int NWAVE = BLK / 64;  // waves per block
static_assert(NWAVE == 4, "block_sum adds four waves");

// sum over the block (lanes by shuffles, the waves through sh[NWAVE]);
// every thread gets the result
__device__ __forceinline__ float block_sum(float v, float* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  __syncthreads();  // sh may still be read from the previous call
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// Host-side dispatch.  by_dtype calls f(T*) with T the element type `bf16`
// names; the argument only carries T, elem_t recovers it.  by_dtype_width
// adds the access width as a second argument, integral_constant<int, V>:
// 8, 4, 2 or 1 elements for bf16 and 4, 2 or 1 for fp32, any other v
// running as width 1.
template <class F>
void by_dtype(bool bf16, F&& f) {
  if (bf16) f((bf16_t*)nullptr);
  else f((float*)nullptr);
}
template <class P>
using elem_t = std::remove_pointer_t<P>;

template <class F>
void by_dtype_width(bool bf16, int v, F&& f) {
  using std::integral_constant;
  if (bf16 && v == 8) return f((bf16_t*)nullptr, integral_constant<int, 8>{});
  by_dtype(bf16, [&](auto* t) {
    switch (v) {
      case 4: f(t, integral_constant<int, 4>{}); break;
      case 2: f(t, integral_constant<int, 2>{}); break;
      default: f(t, integral_constant<int, 1>{}); break;
    }
  });
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
// kernel; defined in pointwise.hip)
void launch_bump_seed(uintptr_t seed_ptr, hipStream_t stream);
