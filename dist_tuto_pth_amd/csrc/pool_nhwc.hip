// pool_nhwc.hip — K19/K20 on channels-last storage: the general 2-D
// max-pool and the global average pool over [B][H][W][C] tensors (fp32 or
// bf16), forward and backward.  The contract is pool.hip's: fp32
// arithmetic, one rounding per element, no float atomics, every order fixed
// by the shapes alone.
//
// In this storage the C channels of a pixel are contiguous, so a work item
// takes V adjacent channels (16, 8, 4 or 2 bytes: the widest for which
// C % V == 0 and every pointer is aligned, else one element) and treats
// them independently; what one NCHW work item does per element happens here
// per channel of the group, so selection, slot and order of summation per
// element are the NCHW op's and the results are its bits.
//
// K19 — maxpool2d
//   maxpool2d_nhwc_fwd_kernel  one work item per (output pixel, channel
//                              group).  Every window position is one V-wide
//                              load; the V channels are compared on their
//                              own under pool.hip's rule (the first
//                              in-bounds position starts as winner at -inf;
//                              a later one wins when v > m or v is NaN).
//                              The V winners and their V uint8 slots, which
//                              lie in NHWC order like y, are one store each.
//   maxpool2d_nhwc_bwd_kernel  gather form, one work item per (input pixel,
//                              channel group): the covering windows in
//                              ascending (oh, ow) order, summed in fp32;
//                              every element of gx is written.
//   Both keep pool.hip's compile-time instances (3x3 and 2x2 windows, at
//   most 2x2 covering windows), which issue all their loads at once, and a
//   run-time one.  Items are counted per sample (PlanePos), so the index
//   inside a sample fits 32 bits and goes through FastDiv; the flat item
//   index times V is the element offset of the result.
//
// K20 — global average pool [B][H][W][C] -> [B][C]
//   gap_nhwc_fwd_kernel        a block takes one sample and one column tile
//                              of nhwc_tile.h.  Pixel p belongs to row lane
//                              p % L, L a power of two from H*W alone, which
//                              adds its pixels in ascending order; the L
//                              lanes are added in lane order (lane_combine);
//                              the sum is divided once and rounded once.
//                              ResNet's 49 pixels take 16 lanes next to 16
//                              column lanes: 128 bf16 channels per block.
//   gap_nhwc_bwd_kernel        a streaming write of gy[b,c]/(H*W): a thread
//                              computes its V values once per sample in
//                              fp32, rounds them once and stores them to
//                              its pixels.
//
// Bindings are registered from kernels.hip's PYBIND11_MODULE through
// register_pool_nhwc().

#include "nhwc_tile.h"
#include "pool_shared.h"

#include <pybind11/pybind11.h>

#include <algorithm>
#include <cmath>

namespace {

template <typename T, int V>
__device__ __forceinline__ Vec<T, V> load_raw(const T* p) {
  Vec<T, V> u;
  u.raw = *reinterpret_cast<const typename Raw<sizeof(T) * V>::type*>(p);
  return u;
}

template <typename T, int V>
__device__ __forceinline__ void store_raw(T* p, const Vec<T, V>& u) {
  *reinterpret_cast<typename Raw<sizeof(T) * V>::type*>(p) = u.raw;
}

// ===========================================================================
// K19 — max-pool
// ===========================================================================
template <typename T, int V, int KH, int KW>
__global__ __launch_bounds__(BLK) void maxpool2d_nhwc_fwd_kernel(
    const T* __restrict__ x, T* __restrict__ y, uint8_t* __restrict__ slot,
    int64_t B, uint32_t C, FastDiv by_cv, PoolGeom g) {
  const uint32_t cv = C / V;
  const uint32_t len = (uint32_t)g.OH * g.OW * cv;  // items of a sample
  const int64_t in_sample = (int64_t)g.H * g.W * C;
  const int64_t n = B * len;
  const int64_t stride = (int64_t)gridDim.x * BLK;
  int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x;
  for (PlanePos at(i, stride, len); i < n; i += stride, at.advance(len)) {
    const uint32_t pix = by_cv(at.r);
    const uint32_t c = (at.r - pix * cv) * V;
    const int oh = (int)g.by_OW(pix);
    const int ow = (int)(pix - (uint32_t)oh * g.OW);
    const int h0 = oh * g.sh - g.ph, w0 = ow * g.sw - g.pw;
    const T* xp = x + at.p * in_sample + c;
    Vec<T, V> mb;
    Vec<uint8_t, V> win;
    if constexpr (KH > 0) {
      Vec<T, V> e[KH * KW];
#pragma unroll
      for (int r = 0; r < KH; ++r)
#pragma unroll
        for (int s = 0; s < KW; ++s)
          e[r * KW + s] = load_raw<T, V>(
              xp + (uint32_t)(min(max(h0 + r, 0), g.H - 1) * g.W +
                              min(max(w0 + s, 0), g.W - 1)) * C);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        float m = -INFINITY;
        T b = T(0);
        int w = 0;
        bool have = false;  // the first in-bounds position always wins
#pragma unroll
        for (int r = 0; r < KH; ++r)
#pragma unroll
          for (int s = 0; s < KW; ++s) {
            const bool in = (uint32_t)(h0 + r) < (uint32_t)g.H &&
                            (uint32_t)(w0 + s) < (uint32_t)g.W;
            const float v = to_f(e[r * KW + s].e[j]);
            if (in && (!have || v > m || v != v)) {
              m = v;
              b = e[r * KW + s].e[j];
              w = r * KW + s;
              have = true;
            }
          }
        mb.e[j] = b;
        win.e[j] = (uint8_t)w;
      }
    } else {
      // the in-bounds part of the window; never empty (pool_geom)
      const int r0 = max(0, -h0), r1 = min(g.kh, g.H - h0);
      const int s0 = max(0, -w0), s1 = min(g.kw, g.W - w0);
      mb = load_raw<T, V>(xp + (uint32_t)((h0 + r0) * g.W + (w0 + s0)) * C);
      float m[V];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        m[j] = -INFINITY;
        win.e[j] = (uint8_t)(r0 * g.kw + s0);
      }
      for (int r = r0; r < r1; ++r)
        for (int s = s0; s < s1; ++s) {
          const Vec<T, V> e = load_raw<T, V>(
              xp + (uint32_t)((h0 + r) * g.W + (w0 + s)) * C);
#pragma unroll
          for (int j = 0; j < V; ++j) {
            const float v = to_f(e.e[j]);
            if (v > m[j] || v != v) {
              m[j] = v;
              mb.e[j] = e.e[j];
              win.e[j] = (uint8_t)(r * g.kw + s);
            }
          }
        }
    }
    store_raw<T, V>(y + i * V, mb);
    store_raw<uint8_t, V>(slot + i * V, win);
  }
}

template <typename T, int V, int TH, int TW>
__global__ __launch_bounds__(BLK) void maxpool2d_nhwc_bwd_kernel(
    const T* __restrict__ gy, const uint8_t* __restrict__ slot,
    T* __restrict__ gx, int64_t B, uint32_t C, FastDiv by_cv, PoolGeom g) {
  const uint32_t cv = C / V;
  const uint32_t len = (uint32_t)g.H * g.W * cv;  // items of a sample
  const int64_t out_sample = (int64_t)g.OH * g.OW * C;
  const int64_t n = B * len;
  const int64_t stride = (int64_t)gridDim.x * BLK;
  int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x;
  for (PlanePos at(i, stride, len); i < n; i += stride, at.advance(len)) {
    const uint32_t pix = by_cv(at.r);
    const uint32_t c = (at.r - pix * cv) * V;
    const int h = (int)g.by_W(pix);
    const int w = (int)(pix - (uint32_t)h * g.W);
    const int hp = h + g.ph, wp = w + g.pw;
    // windows oh with oh*sh <= hp <= oh*sh + kh - 1, clipped to [0, OH-1]
    const int a = hp - g.kh + 1, b = wp - g.kw + 1;
    const int oh_lo = a <= 0 ? 0 : (int)g.by_sh((uint32_t)(a + g.sh - 1));
    const int ow_lo = b <= 0 ? 0 : (int)g.by_sw((uint32_t)(b + g.sw - 1));
    const int oh_hi = min(g.OH - 1, (int)g.by_sh((uint32_t)hp));
    const int ow_hi = min(g.OW - 1, (int)g.by_sw((uint32_t)wp));
    const int64_t ob = at.p * out_sample + c;
    float acc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = 0.f;
    if constexpr (TH > 0) {
      Vec<uint8_t, V> sl[TH * TW];
      Vec<T, V> gv[TH * TW];
#pragma unroll
      for (int u = 0; u < TH; ++u)
#pragma unroll
        for (int v = 0; v < TW; ++v) {
          const int64_t o = ob + (uint32_t)(min(oh_lo + u, g.OH - 1) * g.OW +
                                            min(ow_lo + v, g.OW - 1)) * C;
          sl[u * TW + v] = load_raw<uint8_t, V>(slot + o);
          gv[u * TW + v] = load_raw<T, V>(gy + o);
        }
#pragma unroll
      for (int u = 0; u < TH; ++u)
#pragma unroll
        for (int v = 0; v < TW; ++v) {
          const int oh = oh_lo + u, ow = ow_lo + v;
          const bool covers = oh <= oh_hi && ow <= ow_hi;
          const int want = (hp - oh * g.sh) * g.kw + (wp - ow * g.sw);
#pragma unroll
          for (int j = 0; j < V; ++j)
            if (covers && (int)sl[u * TW + v].e[j] == want)
              acc[j] += to_f(gv[u * TW + v].e[j]);
        }
    } else {
      for (int oh = oh_lo; oh <= oh_hi; ++oh) {
        const int rs = (hp - oh * g.sh) * g.kw + wp;
        for (int ow = ow_lo; ow <= ow_hi; ++ow) {
          const int64_t o = ob + (uint32_t)(oh * g.OW + ow) * C;
          const Vec<uint8_t, V> sl = load_raw<uint8_t, V>(slot + o);
          const Vec<T, V> gv = load_raw<T, V>(gy + o);
#pragma unroll
          for (int j = 0; j < V; ++j)
            if ((int)sl.e[j] == rs - ow * g.sw) acc[j] += to_f(gv.e[j]);
        }
      }
    }
    store_vec<T, V>(gx + i * V, acc);
  }
}

// ===========================================================================
// K20 — global average pool
// ===========================================================================
template <typename T, int V>
__global__ __launch_bounds__(BLK) void gap_nhwc_fwd_kernel(
    const T* __restrict__ x, T* __restrict__ y, int64_t B, uint32_t HW,
    uint32_t C, int cl_shift) {
  __shared__ float sh[BLK * V];
  const ColTile t = col_tile<V>(blockIdx.x, cl_shift, C);
  const uint32_t L = (uint32_t)BLK >> cl_shift;
  const uint32_t CT = (uint32_t)V << cl_shift;  // channels of a tile
  const uint32_t c0 = blockIdx.x * CT;
  const float cnt = (float)HW;
  // block-uniform loop: every thread reaches the barriers
  for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
    const T* xp = x + b * HW * C + t.c;
    float acc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = 0.f;
    if (t.live) {
#pragma unroll 4
      for (uint32_t p = t.rl; p < HW; p += L) {
        float f[V];
        load_vec<T, V>(xp + (int64_t)p * C, f);
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] += f[j];
      }
    }
    // lane_combine's sum, in its order, but for every channel of the tile:
    // with fewer row lanes than V (H*W <= 16) the tile has more channels
    // than the block has threads
    __syncthreads();  // sh may still be read from the previous sample
#pragma unroll
    for (int j = 0; j < V; ++j) sh[t.rl * CT + t.cl * V + j] = acc[j];
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < CT && c0 + i < C; i += BLK) {
      float s = sh[i];
      for (uint32_t r = 1; r < L; ++r) s += sh[r * CT + i];
      from_f(s / cnt, y[b * C + c0 + i]);
    }
  }
}

template <typename T, int V>
__global__ __launch_bounds__(BLK) void gap_nhwc_bwd_kernel(
    const T* __restrict__ gy, T* __restrict__ gx, int64_t B, uint32_t HW,
    uint32_t C, int cl_shift) {
  const ColTile t = col_tile<V>(blockIdx.x, cl_shift, C);
  if (!t.live) return;
  const uint32_t RL = (uint32_t)BLK >> cl_shift;
  const float cnt = (float)HW;
  for (int64_t b = blockIdx.z; b < B; b += gridDim.z) {
    float f[V];
    load_vec<T, V>(gy + b * C + t.c, f);
    Vec<T, V> u;
#pragma unroll
    for (int j = 0; j < V; ++j) from_f(f[j] / cnt, u.e[j]);
    T* gp = gx + b * HW * C + t.c;
    for (uint32_t p = blockIdx.y * RL + t.rl; p < HW; p += gridDim.y * RL)
      store_raw<T, V>(gp + (int64_t)p * C, u);
  }
}

// ===========================================================================
// host launchers
// ===========================================================================
// The geometry and pool.hip's guards, plus what this layout indexes in 32
// bits: the elements of one sample, and C as a FastDiv divisor.
PoolGeom nhwc_geom(const char* who, int64_t B, int64_t C, int64_t H,
                   int64_t W, int64_t kh, int64_t kw, int64_t sh, int64_t sw,
                   int64_t ph, int64_t pw) {
  const PoolGeom g = pool_geom(who, B, C, H, W, kh, kw, sh, sw, ph, pw);
  if (C > POOL_MAX_PLANE || H * W * C >= ((int64_t)1 << 31) ||
      (int64_t)g.OH * g.OW * C >= ((int64_t)1 << 31))
    throw std::invalid_argument(
        std::string(who) + ": a sample has too many elements for the "
                           "channels-last kernel's 32-bit index");
  return g;
}

// pick_v for the tensors of T, narrowed until the uint8 slots are aligned
int pick_v_slots(int es, int64_t C, uintptr_t a, uintptr_t b,
                 uintptr_t slot) {
  int v = pick_v(es, C, {a, b});
  while (slot % (uintptr_t)v) v >>= 1;
  return v;
}

// y [B][OH][OW][C] and slot (uint8, same order) are fully written
void maxpool2d_nhwc_fwd(uintptr_t x, uintptr_t y, uintptr_t slot, int64_t B,
                        int64_t C, int64_t H, int64_t W, int64_t kh,
                        int64_t kw, int64_t sh, int64_t sw, int64_t ph,
                        int64_t pw, bool bf16, uintptr_t stream) {
  const PoolGeom g =
      nhwc_geom("maxpool2d_nhwc_fwd", B, C, H, W, kh, kw, sh, sw, ph, pw);
  if (!x || !y || !slot)
    throw std::invalid_argument("maxpool2d_nhwc_fwd: null tensor");
  const int v = pick_v_slots(bf16 ? 2 : 4, C, x, y, slot);
  const int64_t n = B * g.OH * g.OW * (C / v);
  by_dtype_width(bf16, v, [&](auto* t, auto vv) {
    using T = elem_t<decltype(t)>;
    constexpr int V = vv();
    auto kernel = maxpool2d_nhwc_fwd_kernel<T, V, 0, 0>;
    if (kh == 3 && kw == 3) kernel = maxpool2d_nhwc_fwd_kernel<T, V, 3, 3>;
    if (kh == 2 && kw == 2) kernel = maxpool2d_nhwc_fwd_kernel<T, V, 2, 2>;
    hipLaunchKernelGGL(kernel, dim3(grid_for(n, BLK)), dim3(BLK), 0,
                       S(stream), (const T*)x, (T*)y, (uint8_t*)slot, B,
                       (uint32_t)C, FastDiv((uint32_t)(C / V)), g);
  });
  HIP_CHECK(hipGetLastError());
}

// gx [B][H][W][C] is fully written
void maxpool2d_nhwc_bwd(uintptr_t gy, uintptr_t slot, uintptr_t gx, int64_t B,
                        int64_t C, int64_t H, int64_t W, int64_t kh,
                        int64_t kw, int64_t sh, int64_t sw, int64_t ph,
                        int64_t pw, bool bf16, uintptr_t stream) {
  const PoolGeom g =
      nhwc_geom("maxpool2d_nhwc_bwd", B, C, H, W, kh, kw, sh, sw, ph, pw);
  if (!gy || !slot || !gx)
    throw std::invalid_argument("maxpool2d_nhwc_bwd: null tensor");
  const int v = pick_v_slots(bf16 ? 2 : 4, C, gy, gx, slot);
  const int64_t n = B * H * W * (C / v);
  // at most two windows per direction cover an input when k <= 2*s
  const bool few = kh <= 2 * sh && kw <= 2 * sw;
  by_dtype_width(bf16, v, [&](auto* t, auto vv) {
    using T = elem_t<decltype(t)>;
    constexpr int V = vv();
    auto kernel = few ? maxpool2d_nhwc_bwd_kernel<T, V, 2, 2>
                      : maxpool2d_nhwc_bwd_kernel<T, V, 0, 0>;
    hipLaunchKernelGGL(kernel, dim3(grid_for(n, BLK)), dim3(BLK), 0,
                       S(stream), (const T*)gy, (const uint8_t*)slot, (T*)gx,
                       B, (uint32_t)C, FastDiv((uint32_t)(C / V)), g);
  });
  HIP_CHECK(hipGetLastError());
}

void check_gap_nhwc(const char* who, int64_t B, int64_t C, int64_t HW,
                    uintptr_t a, uintptr_t b) {
  if (B < 1 || C < 1)
    throw std::invalid_argument(std::string(who) + ": B and C must be >= 1");
  if (C >= ((int64_t)1 << 31))
    throw std::invalid_argument(std::string(who) + ": too many channels");
  check_gap(who, B * C, HW, a, b);
}

unsigned col_tiles(int64_t C, int v, int cl_shift) {
  const int64_t ct = (int64_t)v << cl_shift;
  return (unsigned)((C + ct - 1) / ct);
}

// x [B][HW][C] -> y [B][C]
void global_avgpool2d_nhwc_fwd(uintptr_t x, uintptr_t y, int64_t B, int64_t C,
                               int64_t HW, bool bf16, uintptr_t stream) {
  check_gap_nhwc("global_avgpool2d_nhwc_fwd", B, C, HW, x, y);
  // L row lanes from H*W alone, at most 32 so that 8 column lanes remain
  int cl_shift = 8;
  for (int L = std::min(gap_lanes(HW), 32); L > 1; L >>= 1) --cl_shift;
  // y is written one element at a time: only x decides the width
  by_dtype_width(bf16, pick_v(bf16 ? 2 : 4, C, {x}), [&](auto* t, auto v) {
    using T = elem_t<decltype(t)>;
    hipLaunchKernelGGL(
        (gap_nhwc_fwd_kernel<T, v()>),
        dim3(col_tiles(C, v(), cl_shift),
             (unsigned)std::min<int64_t>(B, 65535)),
        dim3(BLK), 0, S(stream), (const T*)x, (T*)y, B, (uint32_t)HW,
        (uint32_t)C, cl_shift);
  });
  HIP_CHECK(hipGetLastError());
}

// gy [B][C] -> gx [B][HW][C], fully written
void global_avgpool2d_nhwc_bwd(uintptr_t gy, uintptr_t gx, int64_t B,
                               int64_t C, int64_t HW, bool bf16,
                               uintptr_t stream) {
  check_gap_nhwc("global_avgpool2d_nhwc_bwd", B, C, HW, gy, gx);
  const int cl_shift = nhwc_cl_shift(C);
  const int64_t rl = BLK >> cl_shift;
  const int64_t by = std::min<int64_t>((HW + rl * 4 - 1) / (rl * 4), 64);
  by_dtype_width(bf16, pick_v(bf16 ? 2 : 4, C, {gy, gx}), [&](auto* t,
                                                              auto v) {
    using T = elem_t<decltype(t)>;
    hipLaunchKernelGGL(
        (gap_nhwc_bwd_kernel<T, v()>),
        dim3(col_tiles(C, v(), cl_shift), (unsigned)by,
             (unsigned)std::min<int64_t>(B, 65535)),
        dim3(BLK), 0, S(stream), (const T*)gy, (T*)gx, B, (uint32_t)HW,
        (uint32_t)C, cl_shift);
  });
  HIP_CHECK(hipGetLastError());
}

}  // namespace

void register_pool_nhwc(pybind11::module_& m) {
  m.def("maxpool2d_nhwc_fwd", &maxpool2d_nhwc_fwd);
  m.def("maxpool2d_nhwc_bwd", &maxpool2d_nhwc_bwd);
  m.def("global_avgpool2d_nhwc_fwd", &global_avgpool2d_nhwc_fwd);
  m.def("global_avgpool2d_nhwc_bwd", &global_avgpool2d_nhwc_bwd);
}
