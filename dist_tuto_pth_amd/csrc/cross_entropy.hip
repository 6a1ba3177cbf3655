// cross_entropy.hip — K21: cross-entropy loss over [B,N] logits (fp32 or
// bf16) and int64 targets, with label smoothing, ignore_index and the three
// reductions, forward and backward.
//
// Contract (the CPU path of ops.cross_entropy is the plain-torch form of
// it): all arithmetic is fp32, the loss is fp32 whatever the logits' dtype,
// gx is rounded once to the logits' dtype.  With eps = label_smoothing and
// t = target[b]:
//   row[b]  = lse[b] - (1-eps)*x[b,t] - (eps/N)*sum_i x[b,i]
//   gx[b,i] = (exp(x[b,i] - lse[b]) - q[b,i]) * g,
//             q = (1-eps)*onehot + eps/N
// The smoothing term is left out when eps == 0, so a -inf logit then gives
// p = 0 and a finite loss.  A row with t == ignore_index has row = lse = 0
// and a gx row of stored zeros (its logits are never read).  "mean" divides
// by the number of rows not ignored, counted on the device; no rows give
// 0/0 = NaN.  A NaN logit makes its row's lse and loss NaN, as in torch.
// g is read from device memory: gloss[0] for "sum",
// gloss[0]/count for "mean", gloss[b] for "none".  The forward keeps only
// lse [B] and the count; the backward recomputes the softmax.
//
// Target values: a target outside [0, N) that is not ignore_index stays
// unchecked, because checking it would synchronize with the device.  The
// kernels only ever COMPARE the target with the running column index and
// never use it as an address: a bad label gives a meaningless loss (no
// column is picked) but cannot read or write out of bounds.
//
// Order of operations.  A row is cut into chunks of 8 elements; chunk c
// belongs to lane c % G of the G lanes that own the row and a lane takes
// its chunks in ascending order.  A chunk's 8 exponentials (and its 8
// values, for the smoothing sum) are added as a fixed tree; columns past N
// count as -inf (0 in the sum of x).  Each lane keeps a running maximum m
// and a sum s of exp(x - m), rescaled by exp(m_old - m_new) when the
// maximum moves (online softmax: the row is read once).  Lanes are merged
// by a butterfly of wave shuffles, the four waves of a block through LDS in
// ascending order.  G depends on N alone:
//   N <= WAVE_MAX_N   G = the smallest power of two with 8*G >= N, at most
//                     64: a row per G lanes, 256/G rows per block
//                     (xent_fwd_wave_kernel)
//   larger            G = 256: a block per row, each thread looping over
//                     its chunks (xent_fwd_block_kernel)
// Nothing in that order depends on the access width, the pointers'
// alignment or the dtype: a chunk is read as 16-byte vectors when every
// row starts on a 16-byte boundary (chosen per launch) and element by
// element otherwise, and bf16 widens exactly.  So the bf16 op gives the
// bits of the fp32 op on the widened values, and every result is bitwise
// reproducible: no float atomics anywhere.  Products that feed a sum go
// through __fmul_rn/__fadd_rn, so no instance contracts them differently
// from another.
//
// xent_finish_kernel (one block) sums row [B] and counts the rows not
// ignored, thread i taking rows i, i+256, ... in ascending order, then a
// fixed tree: the order depends on B alone.
// The 8-element access (load_vec / store_vec), the chunk's tree (tree8) and
// by_dtype are common.h's; xent_finish_kernel keeps block_sum's order
// written out, because it reduces a float and an int in one pass.
// xent_bwd_kernel is one pass with the forward's mapping: read x, write gx.
// Limit: a row is never split across blocks, so a few very long rows (B far
// below the number of CUs) use only B blocks of the chip.
//
// Bindings are registered from kernels.hip's PYBIND11_MODULE through
// register_cross_entropy().

#include "common.h"

#include <pybind11/pybind11.h>

#include <cmath>
#include <initializer_list>

namespace {

constexpr int CH = 8;             // elements per chunk
constexpr int WAVE_MAX_N = 2048;  // above: a block per row (measured, see
                                  // profiles/cross_entropy_numbers.md)

// running maximum and rescaled sum of exponentials
struct MS {
  float m, s;
};

// merge of two partial (m, s): symmetric in its arguments, so both sides of
// a butterfly exchange compute the same bits
__device__ __forceinline__ MS merge(MS a, MS b) {
  const float mn = fmaxf(a.m, b.m);
  // nothing finite on either side: 0 + 0, or the NaN of a poisoned side
  if (mn == -INFINITY) return MS{-INFINITY, a.s + b.s};
  const float fa = a.m == mn ? 1.f : __expf(a.m - mn);
  const float fb = b.m == mn ? 1.f : __expf(b.m - mn);
  return MS{mn, __fadd_rn(__fmul_rn(a.s, fa), __fmul_rn(b.s, fb))};
}

// The 8 values of chunk c of the row at xr: v[] for the exponentials (-inf
// past N), z[] for the sum of x (0 past N).  With VEC every row starts on a
// 16-byte boundary, so a whole chunk is one aligned load_vec.
template <typename T, bool VEC>
__device__ __forceinline__ void load_chunk(const T* __restrict__ xr, int c,
                                           int N, float (&v)[CH],
                                           float (&z)[CH]) {
  const int col0 = c * CH;
  if (VEC && col0 + CH <= N) {
    load_vec<T, CH>(xr + col0, v);
#pragma unroll
    for (int j = 0; j < CH; ++j) z[j] = v[j];
  } else {
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const bool in = col0 + j < N;
      const float f = in ? to_f(xr[col0 + j]) : 0.f;
      v[j] = in ? f : -INFINITY;
      z[j] = f;
    }
  }
}

// what a lane knows of its row: (m, s), the sum of x, the picked x[t]
struct Part {
  MS ms;
  float sx, xt;
};

// chunks lane, lane + G, ... of one row
template <typename T, bool VEC>
__device__ __forceinline__ Part scan_row(const T* __restrict__ xr, int N,
                                         int tc, int lane, int G,
                                         int nchunks) {
  Part p{{-INFINITY, 0.f}, 0.f, 0.f};
  for (int c = lane; c < nchunks; c += G) {
    float v[CH], z[CH];
    load_chunk<T, VEC>(xr, c, N, v, z);
    float cm = v[0];
    bool nan = v[0] != v[0];
#pragma unroll
    for (int j = 1; j < CH; ++j) {
      cm = fmaxf(cm, v[j]);     // drops a NaN
      nan |= v[j] != v[j];
    }
    const float mn = fmaxf(p.ms.m, cm);
    if (mn == -INFINITY) {
      // no finite value so far.  A NaN must still reach the loss: it
      // poisons s, which every later rescaling and merge keeps (NaN * 0)
      if (nan) p.ms.s = __builtin_nanf("");
    } else {
      const float f = p.ms.m == mn ? 1.f : __expf(p.ms.m - mn);
      float e[CH];
#pragma unroll
      for (int j = 0; j < CH; ++j) e[j] = __expf(v[j] - mn);
      p.ms.s = __fadd_rn(__fmul_rn(p.ms.s, f), tree8(e));
      p.ms.m = mn;
    }
    p.sx += tree8(z);
    // the target is only compared with the column index
#pragma unroll
    for (int j = 0; j < CH; ++j)
      if (c * CH + j == tc) p.xt = v[j];
  }
  return p;
}

__device__ __forceinline__ Part merge(Part a, Part b) {
  return Part{merge(a.ms, b.ms), a.sx + b.sx, a.xt + b.xt};
}

__device__ __forceinline__ Part shfl_xor(Part p, int o) {
  return Part{{__shfl_xor(p.ms.m, o, 64), __shfl_xor(p.ms.s, o, 64)},
              __shfl_xor(p.sx, o, 64), __shfl_xor(p.xt, o, 64)};
}

// the target as a column to compare with: -1 (no column) when out of range
__device__ __forceinline__ int target_col(int64_t t, int N) {
  return t >= 0 && t < (int64_t)N ? (int)t : -1;
}

__device__ __forceinline__ void write_row(Part p, float eps, int N,
                                          float* __restrict__ row,
                                          float* __restrict__ lse,
                                          int64_t b) {
  const float l = p.ms.m + __logf(p.ms.s);
  float r = __fadd_rn(l, -__fmul_rn(1.f - eps, p.xt));
  if (eps != 0.f) r = __fadd_rn(r, -__fmul_rn(eps / (float)N, p.sx));
  row[b] = r;
  lse[b] = l;
}

// L lanes per row, a power of two in 1..64; BLK/L rows per block
template <typename T, bool VEC>
__global__ __launch_bounds__(BLK) void xent_fwd_wave_kernel(
    const T* __restrict__ x, const int64_t* __restrict__ target,
    float* __restrict__ row, float* __restrict__ lse, int B, int N,
    float eps, int64_t ignore, int L) {
  const int lane = threadIdx.x % L;
  const int64_t b = (int64_t)blockIdx.x * (BLK / L) + threadIdx.x / L;
  const bool live = b < B;
  const int64_t t = live ? target[b] : ignore;
  const bool on = live && t != ignore;
  // an ignored or absent row scans nothing, yet reaches every shuffle
  const int nchunks = on ? (N + CH - 1) / CH : 0;
  Part p = scan_row<T, VEC>(x + (on ? b : 0) * N, N, target_col(t, N), lane,
                            L, nchunks);
  for (int o = L >> 1; o > 0; o >>= 1) p = merge(p, shfl_xor(p, o));
  if (lane == 0 && live) {
    if (on) {
      write_row(p, eps, N, row, lse, b);
    } else {
      row[b] = 0.f;
      lse[b] = 0.f;
    }
  }
}

// a block per row
template <typename T, bool VEC>
__global__ __launch_bounds__(BLK) void xent_fwd_block_kernel(
    const T* __restrict__ x, const int64_t* __restrict__ target,
    float* __restrict__ row, float* __restrict__ lse, int B, int N,
    float eps, int64_t ignore) {
  __shared__ Part sh[NWAVE];
  const int64_t b = blockIdx.x;
  const int64_t t = target[b];
  if (t == ignore) {   // block-uniform
    if (threadIdx.x == 0) {
      row[b] = 0.f;
      lse[b] = 0.f;
    }
    return;
  }
  Part p = scan_row<T, VEC>(x + b * N, N, target_col(t, N), threadIdx.x, BLK,
                            (N + CH - 1) / CH);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) p = merge(p, shfl_xor(p, o));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = p;
  __syncthreads();
  if (threadIdx.x == 0) {
    Part r = sh[0];
#pragma unroll
    for (int w = 1; w < NWAVE; ++w) r = merge(r, sh[w]);
    write_row(r, eps, N, row, lse, b);
  }
}

// loss = sum or mean of row [B]; count = rows not ignored (as a float)
__global__ __launch_bounds__(BLK) void xent_finish_kernel(
    const float* __restrict__ row, const int64_t* __restrict__ target,
    float* __restrict__ loss, float* __restrict__ count, int B,
    int64_t ignore, int mean) {
  __shared__ float shs[NWAVE];
  __shared__ int shc[NWAVE];
  float s = 0.f;
  int c = 0;
  for (int64_t i = threadIdx.x; i < B; i += BLK) {
    s += row[i];
    c += target[i] != ignore ? 1 : 0;
  }
  // block_sum's order, written out: the float and the int share one pass
  // through LDS (two block_sum calls cost this one-block kernel 0.2 us)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_down(s, o, 64);
    c += __shfl_down(c, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    shs[threadIdx.x >> 6] = s;
    shc[threadIdx.x >> 6] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float tot = (shs[0] + shs[1]) + (shs[2] + shs[3]);
    const float cnt = (float)((shc[0] + shc[1]) + (shc[2] + shc[3]));
    loss[0] = mean ? tot / cnt : tot;
    count[0] = cnt;
  }
}

enum { RED_NONE = 0, RED_MEAN = 1, RED_SUM = 2 };

// G lanes per row (a power of two, 1..256): BLK/G rows per block
template <typename T, bool VEC>
__global__ __launch_bounds__(BLK) void xent_bwd_kernel(
    const T* __restrict__ x, const int64_t* __restrict__ target,
    const float* __restrict__ lse, const float* __restrict__ count,
    const float* __restrict__ gloss, T* __restrict__ gx, int B, int N,
    float eps, int64_t ignore, int reduction, int G) {
  const int lane = threadIdx.x % G;
  const int64_t b = (int64_t)blockIdx.x * (BLK / G) + threadIdx.x / G;
  if (b >= B) return;
  const int64_t t = target[b];
  const bool on = t != ignore;
  const int tc = target_col(t, N);
  float g = 0.f, l = 0.f;
  if (on) {
    g = reduction == RED_NONE ? gloss[b] : gloss[0];
    if (reduction == RED_MEAN) g = g / count[0];
    l = lse[b];
  }
  const float en = eps / (float)N;
  const float qt = (1.f - eps) + en;
  const T* xr = x + b * N;
  T* gr = gx + b * N;
  const int nchunks = (N + CH - 1) / CH;
  for (int c = lane; c < nchunks; c += G) {
    const int col0 = c * CH;
    float o[CH];
    if (on) {
      float v[CH], z[CH];
      load_chunk<T, VEC>(xr, c, N, v, z);
#pragma unroll
      for (int j = 0; j < CH; ++j)
        o[j] = (__expf(v[j] - l) - (col0 + j == tc ? qt : en)) * g;
    } else {
#pragma unroll
      for (int j = 0; j < CH; ++j) o[j] = 0.f;   // stored, not 0*g
    }
    if (VEC && col0 + CH <= N) {
      store_vec<T, CH>(gr + col0, o);
    } else {
#pragma unroll
      for (int j = 0; j < CH; ++j)
        if (col0 + j < N) from_f(o[j], gr[col0 + j]);
    }
  }
}

// ===========================================================================
// host launchers
// ===========================================================================
// lanes per row from N alone; `mapping` 1 (lanes of a wave) or 2 (a block)
// overrides the threshold, for measuring it
int lanes_for(int64_t N, int mapping) {
  if (mapping == 2 || (mapping == 0 && N > WAVE_MAX_N)) return BLK;
  int L = 1;
  while (L < 64 && (int64_t)L * CH < N) L *= 2;
  return L;
}

void check_xent(const char* who, int64_t B, int64_t N, int reduction,
                int mapping, int es, std::initializer_list<uintptr_t> elems,
                std::initializer_list<uintptr_t> others) {
  const std::string op(who);
  if (B < 1 || N < 1)
    throw std::invalid_argument(op + ": B and N must be >= 1");
  if (B > INT32_MAX || N > INT32_MAX - 2 * CH * BLK)
    throw std::invalid_argument(op + ": B or N does not fit 32 bits");
  if (reduction < RED_NONE || reduction > RED_SUM)
    throw std::invalid_argument(op + ": reduction must be 0, 1 or 2");
  if (mapping < 0 || mapping > 2)
    throw std::invalid_argument(op + ": mapping must be 0, 1 or 2");
  for (uintptr_t p : elems)
    if (!p || p % es)
      throw std::invalid_argument(
          op + ": null tensor or one not aligned to its element size");
  for (uintptr_t p : others)
    if (!p || p % 4)
      throw std::invalid_argument(op + ": null or misaligned tensor");
}

// row [B] and lse [B] (fp32) are fully written; loss [1] and count [1]
// (fp32) too unless reduction is 0 ("none"), which does not touch them
void cross_entropy_fwd(uintptr_t x, uintptr_t target, uintptr_t row,
                       uintptr_t lse, uintptr_t loss, uintptr_t count,
                       int64_t B, int64_t N, double eps, int64_t ignore,
                       int reduction, bool bf16, int mapping,
                       uintptr_t stream) {
  const int es = bf16 ? 2 : 4;
  check_xent("cross_entropy_fwd", B, N, reduction, mapping, es, {x},
             {row, lse});
  if (!target || target % 8)
    throw std::invalid_argument("cross_entropy_fwd: bad target pointer");
  if (reduction != RED_NONE && (!loss || !count || loss % 4 || count % 4))
    throw std::invalid_argument("cross_entropy_fwd: bad loss or count");
  const bool vec = x % 16 == 0 && (N * es) % 16 == 0;
  const int G = lanes_for(N, mapping);
  by_dtype(bf16, [&](auto* tp) {
    using T = elem_t<decltype(tp)>;
    if (G == BLK) {
      auto kernel = vec ? xent_fwd_block_kernel<T, true>
                        : xent_fwd_block_kernel<T, false>;
      hipLaunchKernelGGL(kernel, dim3((unsigned)B), dim3(BLK), 0, S(stream),
                         (const T*)x, (const int64_t*)target, (float*)row,
                         (float*)lse, (int)B, (int)N, (float)eps, ignore);
    } else {
      auto kernel = vec ? xent_fwd_wave_kernel<T, true>
                        : xent_fwd_wave_kernel<T, false>;
      const int rpb = BLK / G;
      hipLaunchKernelGGL(kernel, dim3((unsigned)((B + rpb - 1) / rpb)),
                         dim3(BLK), 0, S(stream), (const T*)x,
                         (const int64_t*)target, (float*)row, (float*)lse,
                         (int)B, (int)N, (float)eps, ignore, G);
    }
  });
  HIP_CHECK(hipGetLastError());
  if (reduction != RED_NONE) {
    hipLaunchKernelGGL(xent_finish_kernel, dim3(1), dim3(BLK), 0, S(stream),
                       (const float*)row, (const int64_t*)target,
                       (float*)loss, (float*)count, (int)B, ignore,
                       reduction == RED_MEAN ? 1 : 0);
    HIP_CHECK(hipGetLastError());
  }
}

// gx [B,N] is fully written.  gloss is [1] (fp32), or [B] for reduction 0;
// count [1] is read for reduction 1 ("mean") only.
void cross_entropy_bwd(uintptr_t x, uintptr_t target, uintptr_t lse,
                       uintptr_t count, uintptr_t gloss, uintptr_t gx,
                       int64_t B, int64_t N, double eps, int64_t ignore,
                       int reduction, bool bf16, int mapping,
                       uintptr_t stream) {
  const int es = bf16 ? 2 : 4;
  check_xent("cross_entropy_bwd", B, N, reduction, mapping, es, {x, gx},
             {lse, gloss});
  if (!target || target % 8)
    throw std::invalid_argument("cross_entropy_bwd: bad target pointer");
  if (reduction == RED_MEAN && (!count || count % 4))
    throw std::invalid_argument("cross_entropy_bwd: bad count pointer");
  const bool vec = x % 16 == 0 && gx % 16 == 0 && (N * es) % 16 == 0;
  const int G = lanes_for(N, mapping);
  const int rpb = BLK / G;
  by_dtype(bf16, [&](auto* tp) {
    using T = elem_t<decltype(tp)>;
    auto kernel = vec ? xent_bwd_kernel<T, true> : xent_bwd_kernel<T, false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((B + rpb - 1) / rpb)),
                       dim3(BLK), 0, S(stream), (const T*)x,
                       (const int64_t*)target, (const float*)lse,
                       (const float*)count, (const float*)gloss, (T*)gx,
                       (int)B, (int)N, (float)eps, ignore, reduction, G);
  });
  HIP_CHECK(hipGetLastError());
}

int cross_entropy_wave_max_n() { return WAVE_MAX_N; }

}  // namespace

void register_cross_entropy(pybind11::module_& m) {
  m.def("cross_entropy_fwd", &cross_entropy_fwd);
  m.def("cross_entropy_bwd", &cross_entropy_bwd);
  m.def("cross_entropy_wave_max_n", &cross_entropy_wave_max_n);
}
