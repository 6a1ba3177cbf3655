// pool.hip — K19/K20: general 2-D max-pool and global average pool over
// NCHW tensors (fp32 or bf16), forward and backward.
//
// Contract (the CPU paths of ops.maxpool2d and ops.global_avgpool2d are the
// plain-torch form of it): all arithmetic is fp32, every output element is
// rounded once to its dtype, nothing uses float atomics and every sum has
// an order fixed by the shapes alone, so every result is bitwise
// reproducible and does not depend on the alignment of the base pointers.
//
// K19 — maxpool2d(kernel, stride, padding), windows may overlap.
//   maxpool2d_fwd_kernel   one work item per output.  Padding acts as -inf
//                          and is never selected.  The window is scanned
//                          row-major over its in-bounds positions, starting
//                          from the first one as winner at value -inf; a
//                          later position wins when v > m or v is NaN
//                          (torch's rule: the first maximum wins a tie, an
//                          all -inf window selects its first element, NaN
//                          propagates).  The output carries the winner's
//                          bits; its window slot r*kw + s is saved as one
//                          uint8 per output (kh*kw <= 256).
//   maxpool2d_bwd_kernel   gather form, one work item per INPUT element: it
//                          visits the windows that cover it, adds gy where
//                          the saved slot names it, in ascending (oh, ow)
//                          order, and writes every element of gx (zeros
//                          where no window selects or covers it), so gx
//                          needs no pre-zeroing.
//   Both have an instance with compile-time extents for the common small
//   cases (3x3 and 2x2 windows forward, at most 2x2 covering windows
//   backward), which issues all its loads at once, and a run-time one.
//
// K20 — global average pool [B,C,H,W] -> [B,C].
//   gap_fwd_wave_kernel    planes of at most WAVE_MAX_HW elements: L lanes
//                          per plane (a power of two, 1..64, from H*W
//                          alone), so a wave reduces 64/L neighbouring
//                          planes at once — ResNet's 131072 planes of 49
//                          elements take 16 lanes each.  Element e belongs
//                          to lane e % L, which adds its elements in
//                          ascending order; the L lanes are summed by a
//                          butterfly of wave shuffles.
//   gap_fwd_block_kernel   larger planes: a block per plane.  Element e
//                          belongs to thread e % 256 and to its accumulator
//                          (e / 256) % 4; the four are added as a fixed
//                          tree, the lanes by shuffles, the waves through
//                          LDS (block_sum of common.h).
//   gap_bwd_kernel         gx[b,c,:,:] = float(gy[b,c]) / (H*W): a streaming
//                          write in 16-byte accesses (Vec of common.h)
//                          between a scalar head (up to gx's first 16-byte
//                          boundary) and tail.
//   Both forward kernels read one element per access, so the order above is
//   the only thing that decides the bits.  Limit: a plane is never split
//   across blocks, so a few huge planes (B*C far below the number of CUs)
//   use only B*C blocks of the chip.
//
// Grid-stride loops over int64 flat indices, 256-thread blocks, grids
// capped by grid_for(), launchers dispatched on the dtype by common.h's
// by_dtype.  Bindings are registered from kernels.hip's
// PYBIND11_MODULE through register_pool().

#include "common.h"

#include <pybind11/pybind11.h>

#include <algorithm>
#include <cmath>

namespace {

constexpr uint32_t WAVE_MAX_HW = 1024;  // above: a block per plane

// ===========================================================================
// K19 — max-pool
// ===========================================================================
// n / d for 0 <= n < 2^31 and 1 <= d <= 2^29 without a hardware division
// (Granlund and Montgomery's multiply and shift, rounded-up multiplier):
// with s = ceil(log2 d) and m = floor(2^32 * (2^s - d) / d) + 1,
// n / d = (mulhi(n, m) + n) >> s.  The element-index divisions are most of
// the arithmetic of these kernels, which are otherwise a few loads.
struct FastDiv {
  uint32_t m, s;

  FastDiv() = default;
  explicit FastDiv(uint32_t d) {
    s = 0;
    while (((uint64_t)1 << s) < d) ++s;
    m = (uint32_t)((((uint64_t)1 << 32) * (((uint64_t)1 << s) - d)) / d + 1);
  }
  __device__ __forceinline__ uint32_t operator()(uint32_t n) const {
    return (__umulhi(n, m) + n) >> s;
  }
};

struct PoolGeom {
  int H, W, OH, OW, kh, kw, sh, sw, ph, pw;
  FastDiv by_W, by_OW, by_sh, by_sw;
};

// Position of a grid-stride loop over planes of `len` elements: the flat
// index is p*len + r.  One 64-bit division per thread, none per element.
struct PlanePos {
  int64_t p;
  uint32_t r;
  int64_t step_p;
  uint32_t step_r;

  __device__ __forceinline__ PlanePos(int64_t i, int64_t stride,
                                      uint32_t len) {
    p = i / len;
    r = (uint32_t)(i - p * len);
    step_p = stride / len;
    step_r = (uint32_t)(stride - step_p * len);
  }
  __device__ __forceinline__ void advance(uint32_t len) {
    p += step_p;
    r += step_r;  // both below len < 2^31
    if (r >= len) {
      r -= len;
      ++p;
    }
  }
};

// KH x KW is the window when KH > 0, and g.kh x g.kw at run time when
// KH == 0.  With a compile-time window every position is loaded at once,
// an out-of-bounds one from a clamped (valid) address and then ignored, so
// the loads are independent and in flight together; the run-time scan loads
// one position after the other and is bound by their latency.
template <typename T, int KH, int KW>
__global__ __launch_bounds__(BLK) void maxpool2d_fwd_kernel(
    const T* __restrict__ x, T* __restrict__ y, uint8_t* __restrict__ slot,
    int64_t planes, PoolGeom g) {
  const uint32_t hw = (uint32_t)g.H * g.W, ohw = (uint32_t)g.OH * g.OW;
  const int64_t n = planes * ohw;
  const int64_t stride = (int64_t)gridDim.x * BLK;
  int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x;
  for (PlanePos at(i, stride, ohw); i < n; i += stride, at.advance(ohw)) {
    const int oh = (int)g.by_OW(at.r);
    const int ow = (int)(at.r - (uint32_t)oh * g.OW);
    const int h0 = oh * g.sh - g.ph, w0 = ow * g.sw - g.pw;
    const T* xp = x + at.p * hw;
    T mb = T(0);
    float m = -INFINITY;
    int win = 0;
    if constexpr (KH > 0) {
      T e[KH * KW];
#pragma unroll
      for (int r = 0; r < KH; ++r)
#pragma unroll
        for (int s = 0; s < KW; ++s)
          e[r * KW + s] = xp[min(max(h0 + r, 0), g.H - 1) * g.W +
                             min(max(w0 + s, 0), g.W - 1)];
      bool have = false;  // the first in-bounds position always wins
#pragma unroll
      for (int r = 0; r < KH; ++r)
#pragma unroll
        for (int s = 0; s < KW; ++s) {
          const bool in = (uint32_t)(h0 + r) < (uint32_t)g.H &&
                          (uint32_t)(w0 + s) < (uint32_t)g.W;
          const float v = to_f(e[r * KW + s]);
          if (in && (!have || v > m || v != v)) {
            m = v;
            mb = e[r * KW + s];
            win = r * KW + s;
            have = true;
          }
        }
    } else {
      // the in-bounds part of the window; never empty (kernel > padding
      // and the window fits the padded input, checked by the launcher)
      const int r0 = max(0, -h0), r1 = min(g.kh, g.H - h0);
      const int s0 = max(0, -w0), s1 = min(g.kw, g.W - w0);
      mb = xp[(h0 + r0) * g.W + (w0 + s0)];
      win = r0 * g.kw + s0;
      for (int r = r0; r < r1; ++r) {
        const T* row = xp + (h0 + r) * g.W + w0;
        for (int s = s0; s < s1; ++s) {
          const T e = row[s];
          const float v = to_f(e);
          if (v > m || v != v) {
            m = v;
            mb = e;
            win = r * g.kw + s;
          }
        }
      }
    }
    y[i] = mb;
    slot[i] = (uint8_t)win;
  }
}

// An input element is covered by at most ceil(kh/sh) x ceil(kw/sw) windows.
// TH x TW bounds that count when TH > 0: all slots and gradients are then
// loaded at once (a window past the last covering one from a clamped, valid
// address, and ignored); TH == 0 loops over the covering windows at run
// time, one dependent pair of loads after the other.
template <typename T, int TH, int TW>
__global__ __launch_bounds__(BLK) void maxpool2d_bwd_kernel(
    const T* __restrict__ gy, const uint8_t* __restrict__ slot,
    T* __restrict__ gx, int64_t planes, PoolGeom g) {
  const uint32_t hw = (uint32_t)g.H * g.W, ohw = (uint32_t)g.OH * g.OW;
  const int64_t n = planes * hw;
  const int64_t stride = (int64_t)gridDim.x * BLK;
  int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x;
  for (PlanePos at(i, stride, hw); i < n; i += stride, at.advance(hw)) {
    const int h = (int)g.by_W(at.r);
    const int w = (int)(at.r - (uint32_t)h * g.W);
    const int hp = h + g.ph, wp = w + g.pw;
    // windows oh with oh*sh <= hp <= oh*sh + kh - 1, clipped to [0, OH-1]
    const int a = hp - g.kh + 1, b = wp - g.kw + 1;
    const int oh_lo = a <= 0 ? 0 : (int)g.by_sh((uint32_t)(a + g.sh - 1));
    const int ow_lo = b <= 0 ? 0 : (int)g.by_sw((uint32_t)(b + g.sw - 1));
    const int oh_hi = min(g.OH - 1, (int)g.by_sh((uint32_t)hp));
    const int ow_hi = min(g.OW - 1, (int)g.by_sw((uint32_t)wp));
    const int64_t ob = at.p * ohw;
    float acc = 0.f;
    if constexpr (TH > 0) {
      int sl[TH * TW];
      T gv[TH * TW];
#pragma unroll
      for (int u = 0; u < TH; ++u)
#pragma unroll
        for (int v = 0; v < TW; ++v) {
          const int64_t o = ob + min(oh_lo + u, g.OH - 1) * g.OW +
                            min(ow_lo + v, g.OW - 1);
          sl[u * TW + v] = slot[o];
          gv[u * TW + v] = gy[o];
        }
#pragma unroll
      for (int u = 0; u < TH; ++u)
#pragma unroll
        for (int v = 0; v < TW; ++v) {
          const int oh = oh_lo + u, ow = ow_lo + v;
          if (oh <= oh_hi && ow <= ow_hi &&
              sl[u * TW + v] ==
                  (hp - oh * g.sh) * g.kw + (wp - ow * g.sw))
            acc += to_f(gv[u * TW + v]);
        }
    } else {
      for (int oh = oh_lo; oh <= oh_hi; ++oh) {
        const int rs = (hp - oh * g.sh) * g.kw + wp;
        for (int ow = ow_lo; ow <= ow_hi; ++ow) {
          const int64_t o = ob + oh * g.OW + ow;
          if ((int)slot[o] == rs - ow * g.sw) acc += to_f(gy[o]);
        }
      }
    }
    from_f(acc, gx[i]);
  }
}

// ===========================================================================
// K20 — global average pool
// ===========================================================================
template <typename T>
__global__ __launch_bounds__(BLK) void gap_fwd_wave_kernel(
    const T* __restrict__ x, T* __restrict__ y, int64_t planes, uint32_t hw,
    int L) {
  const int ppb = BLK / L;  // planes per block
  const int sub = threadIdx.x / L;
  const uint32_t lane = threadIdx.x % L;
  const float cnt = (float)hw;
  // block-uniform loop: every lane of a wave reaches the shuffles
  for (int64_t gI = blockIdx.x; gI * ppb < planes; gI += gridDim.x) {
    const int64_t pl = gI * ppb + sub;
    float s = 0.f;
    if (pl < planes) {
      const T* xp = x + pl * hw;
      for (uint32_t e = lane; e < hw; e += L) s += to_f(xp[e]);
    }
    for (int o = L >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0 && pl < planes) from_f(s / cnt, y[pl]);
  }
}

template <typename T>
__global__ __launch_bounds__(BLK) void gap_fwd_block_kernel(
    const T* __restrict__ x, T* __restrict__ y, int64_t planes,
    uint32_t hw) {
  __shared__ float sh[NWAVE];
  const float cnt = (float)hw;
  for (int64_t pl = blockIdx.x; pl < planes; pl += gridDim.x) {
    const T* xp = x + pl * hw;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    uint32_t e = threadIdx.x;
    for (; e + 3 * BLK < hw; e += 4 * BLK) {
      a0 += to_f(xp[e]);
      a1 += to_f(xp[e + BLK]);
      a2 += to_f(xp[e + 2 * BLK]);
      a3 += to_f(xp[e + 3 * BLK]);
    }
    if (e < hw) a0 += to_f(xp[e]);
    if (e + BLK < hw) a1 += to_f(xp[e + BLK]);
    if (e + 2 * BLK < hw) a2 += to_f(xp[e + 2 * BLK]);
    const float v = block_sum((a0 + a1) + (a2 + a3), sh);
    if (threadIdx.x == 0) from_f(v / cnt, y[pl]);
  }
}

template <typename T>
__global__ __launch_bounds__(BLK) void gap_bwd_kernel(
    const T* __restrict__ gy, T* __restrict__ gx, int64_t n, uint32_t hw,
    int64_t head, int64_t nvec) {
  constexpr int V = 16 / sizeof(T);
  const float cnt = (float)hw;
  const int64_t tid = (int64_t)blockIdx.x * BLK + threadIdx.x;
  const int64_t nth = (int64_t)gridDim.x * BLK;
  for (int64_t q = tid; q < nvec; q += nth) {
    const int64_t first = head + q * V;
    int64_t p = first / hw;
    uint32_t r = (uint32_t)(first - p * hw);
    float val = to_f(gy[p]) / cnt;
    Vec<T, V> u;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      if (r == hw) {  // the vector crosses into the next plane
        r = 0;
        val = to_f(gy[++p]) / cnt;
      }
      from_f(val, u.e[j]);
      ++r;
    }
    *reinterpret_cast<uint4*>(gx + first) = u.raw;
  }
  // scalar head [0, head) and tail [head + nvec*V, n): fewer than 2*V
  const int64_t tail = head + nvec * V;
  for (int64_t i = tid; i < head + (n - tail); i += nth) {
    const int64_t at = i < head ? i : tail + (i - head);
    from_f(to_f(gy[at / hw]) / cnt, gx[at]);
  }
}

// ===========================================================================
// host launchers
// ===========================================================================
// planes are indexed in 32 bits; the bound leaves room for the padded and
// strided forms of the index ((H+1)*(W+1) outputs, hp + sh) in an int
constexpr int64_t MAX_PLANE = (int64_t)1 << 29;
constexpr int64_t MAX_ELEMS = (int64_t)1 << 62;

PoolGeom pool_geom(const char* who, int64_t B, int64_t C, int64_t H,
                   int64_t W, int64_t kh, int64_t kw, int64_t sh, int64_t sw,
                   int64_t ph, int64_t pw) {
  const std::string op(who);
  if (B < 1 || C < 1 || H < 1 || W < 1)
    throw std::invalid_argument(op + ": every dimension must be >= 1");
  if (kh < 1 || kw < 1 || sh < 1 || sw < 1 || ph < 0 || pw < 0)
    throw std::invalid_argument(
        op + ": kernel and stride must be >= 1, padding >= 0");
  if (kh * kw > 256 || kh > 256 || kw > 256)
    throw std::invalid_argument(
        op + ": kh*kw must be <= 256 (the window slot is saved as uint8)");
  if (ph > kh / 2 || pw > kw / 2)
    throw std::invalid_argument(
        op + ": padding must be at most half the kernel size");
  if (H + 2 * ph < kh || W + 2 * pw < kw)
    throw std::invalid_argument(
        op + ": the window does not fit the padded input");
  const int64_t OH = (H + 2 * ph - kh) / sh + 1;
  const int64_t OW = (W + 2 * pw - kw) / sw + 1;
  if (H * W > MAX_PLANE || sh > MAX_PLANE || sw > MAX_PLANE ||
      B * C > MAX_ELEMS / (H * W))
    throw std::invalid_argument(op + ": too many elements");
  PoolGeom g;
  g.H = (int)H; g.W = (int)W; g.OH = (int)OH; g.OW = (int)OW;
  g.kh = (int)kh; g.kw = (int)kw; g.sh = (int)sh; g.sw = (int)sw;
  g.ph = (int)ph; g.pw = (int)pw;
  g.by_W = FastDiv((uint32_t)W); g.by_OW = FastDiv((uint32_t)OW);
  g.by_sh = FastDiv((uint32_t)sh); g.by_sw = FastDiv((uint32_t)sw);
  return g;
}

// y [B,C,OH,OW] and slot (uint8, same shape) are fully written
void maxpool2d_fwd(uintptr_t x, uintptr_t y, uintptr_t slot, int64_t B,
                   int64_t C, int64_t H, int64_t W, int64_t kh, int64_t kw,
                   int64_t sh, int64_t sw, int64_t ph, int64_t pw, bool bf16,
                   uintptr_t stream) {
  const PoolGeom g =
      pool_geom("maxpool2d_fwd", B, C, H, W, kh, kw, sh, sw, ph, pw);
  if (!x || !y || !slot)
    throw std::invalid_argument("maxpool2d_fwd: null tensor");
  const int64_t n = B * C * g.OH * g.OW;
  by_dtype(bf16, [&](auto* t) {
    using T = elem_t<decltype(t)>;
    auto kernel = maxpool2d_fwd_kernel<T, 0, 0>;
    if (kh == 3 && kw == 3) kernel = maxpool2d_fwd_kernel<T, 3, 3>;
    if (kh == 2 && kw == 2) kernel = maxpool2d_fwd_kernel<T, 2, 2>;
    hipLaunchKernelGGL(kernel, dim3(grid_for(n, BLK)), dim3(BLK), 0,
                       S(stream), (const T*)x, (T*)y, (uint8_t*)slot, B * C,
                       g);
  });
  HIP_CHECK(hipGetLastError());
}

// gx [B,C,H,W] is fully written
void maxpool2d_bwd(uintptr_t gy, uintptr_t slot, uintptr_t gx, int64_t B,
                   int64_t C, int64_t H, int64_t W, int64_t kh, int64_t kw,
                   int64_t sh, int64_t sw, int64_t ph, int64_t pw, bool bf16,
                   uintptr_t stream) {
  const PoolGeom g =
      pool_geom("maxpool2d_bwd", B, C, H, W, kh, kw, sh, sw, ph, pw);
  if (!gy || !slot || !gx)
    throw std::invalid_argument("maxpool2d_bwd: null tensor");
  const int64_t n = B * C * H * W;
  // at most two windows per direction cover an input when k <= 2*s
  const bool few = kh <= 2 * sh && kw <= 2 * sw;
  by_dtype(bf16, [&](auto* t) {
    using T = elem_t<decltype(t)>;
    auto kernel = few ? maxpool2d_bwd_kernel<T, 2, 2>
                      : maxpool2d_bwd_kernel<T, 0, 0>;
    hipLaunchKernelGGL(kernel, dim3(grid_for(n, BLK)), dim3(BLK), 0,
                       S(stream), (const T*)gy, (const uint8_t*)slot,
                       (T*)gx, B * C, g);
  });
  HIP_CHECK(hipGetLastError());
}

void check_gap(const char* who, int64_t planes, int64_t HW, uintptr_t a,
               uintptr_t b) {
  const std::string op(who);
  if (planes < 1 || HW < 1)
    throw std::invalid_argument(op + ": B*C and H*W must be >= 1");
  if (HW > MAX_PLANE || planes > MAX_ELEMS / HW)
    throw std::invalid_argument(op + ": too many elements");
  if (!a || !b) throw std::invalid_argument(op + ": null tensor");
}

// lanes per plane of gap_fwd_wave_kernel: about four elements per lane
int gap_lanes(int64_t HW) {
  int L = 1;
  while (L < 64 && (int64_t)L * 4 < HW) L *= 2;
  return L;
}

void global_avgpool2d_fwd(uintptr_t x, uintptr_t y, int64_t planes,
                          int64_t HW, bool bf16, uintptr_t stream) {
  check_gap("global_avgpool2d_fwd", planes, HW, x, y);
  by_dtype(bf16, [&](auto* t) {
    using T = elem_t<decltype(t)>;
    if (HW <= (int64_t)WAVE_MAX_HW) {
      const int L = gap_lanes(HW);
      hipLaunchKernelGGL(gap_fwd_wave_kernel<T>,
                         dim3(grid_for(planes * L, BLK)), dim3(BLK), 0,
                         S(stream), (const T*)x, (T*)y, planes, (uint32_t)HW,
                         L);
    } else {
      hipLaunchKernelGGL(gap_fwd_block_kernel<T>,
                         dim3((unsigned)std::min<int64_t>(planes, 4096)),
                         dim3(BLK), 0, S(stream), (const T*)x, (T*)y, planes,
                         (uint32_t)HW);
    }
  });
  HIP_CHECK(hipGetLastError());
}

void global_avgpool2d_bwd(uintptr_t gy, uintptr_t gx, int64_t planes,
                          int64_t HW, bool bf16, uintptr_t stream) {
  check_gap("global_avgpool2d_bwd", planes, HW, gy, gx);
  const int64_t n = planes * HW;
  const int es = bf16 ? 2 : 4, V = 16 / es;
  if (gx % es)
    throw std::invalid_argument(
        "global_avgpool2d_bwd: gx is not aligned to its element size");
  // elements in front of gx's first 16-byte boundary
  const int64_t head = std::min<int64_t>(n, (16 - gx % 16) % 16 / es);
  const int64_t nvec = (n - head) / V;
  by_dtype(bf16, [&](auto* t) {
    using T = elem_t<decltype(t)>;
    hipLaunchKernelGGL(gap_bwd_kernel<T>,
                       dim3(grid_for(std::max<int64_t>(nvec, 2 * V), BLK)),
                       dim3(BLK), 0, S(stream), (const T*)gy, (T*)gx, n,
                       (uint32_t)HW, head, nvec);
  });
  HIP_CHECK(hipGetLastError());
}

}  // namespace

void register_pool(pybind11::module_& m) {
  m.def("maxpool2d_fwd", &maxpool2d_fwd);
  m.def("maxpool2d_bwd", &maxpool2d_bwd);
  m.def("global_avgpool2d_fwd", &global_avgpool2d_fwd);
  m.def("global_avgpool2d_bwd", &global_avgpool2d_bwd);
}
