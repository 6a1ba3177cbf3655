// K17 — bf16 convolution on the CDNA4 matrix cores (gfx950).
//
// Numeric contract (ops.conv2d_bf16) is linear_bf16's: every GEMM operand
// is bf16, products accumulate in fp32 on v_mfma_f32_16x16x32_bf16, each
// result is rounded ONCE (RNE) to its output dtype, padding contributes
// exact zeros.
//
// The three products are implicit GEMMs on the tile core of gemm_bf16.h;
// no im2col buffer exists in global memory, the loaders gather straight
// into the LDS tiles.  NCHW, stride (sh,sw) >= 1, zero padding (ph,pw):
//
//   product   rows M      cols N    reduction        A                B
//   forward   B*OH*OW     K         C*R*S            x gathered (T)   w plain
//   gx        B*H*W       C         K*R*S            gy gathered (T)  w gathered
//   gw (+gb)  K           C*R*S     B*OH*OW, split   gy rows          x gathered
//
// "gathered" is conv_gather8: 8 consecutive pixels of one filter tap.  With
// stride 1 along w they are 8 consecutive addresses of one input row, so
// the chunk runs along the pixel axis: one 16-byte load where the address
// is 16-byte aligned, eight 2-byte loads of one cache line otherwise, and
// a predicated per-element gather at row ends, padding and strides.  (T):
// the chunk runs along the GEMM rows and is transposed on the LDS write,
// as linear_bf16's gw operands are.  The epilogue takes the C tile through
// LDS so that GEMM row m = (b, pixel) goes back to NCHW in runs along the
// pixel axis.
//
// gw is fp32, split over B*OH*OW through a partial buffer that
// gw_combine_kernel sums in split order: no float atomics, bitwise
// reproducible.  gb is the column-sum of the gy tile and rides along.
//
// A chunk (gemm_bf16.h's Chunk) and the epilogue's 8 converted outputs
// (store8) are common.h's Vec: 8 elements that move as one aligned value.
//
// Bindings are registered from kernels.hip's PYBIND11_MODULE through
// register_conv_bf16().

#include "gemm_bf16.h"

#include <pybind11/pybind11.h>

namespace {

// ---------------------------------------------------------------------------
// the gather
// ---------------------------------------------------------------------------
// A "pixel index" m runs over (b, y, x) of a grid Hm x Wm; a "tap" kk runs
// over (ch, r, s).  Forward and gw read x at (y*sh - ph + r, x*sw - pw + s)
// with the grid being the OUTPUT plane.  gx reads gy at
// ((y + ph - r)/sh, (x + pw - s)/sw) where those divide exactly, with the
// grid being the INPUT plane.
struct ConvSrc {
  const bf16_t* p;  // [B, Cs, Hs, Ws]
  int Cs, Hs, Ws;
  int Hm, Wm;       // pixel grid
  int R, S, sh, sw, ph, pw;
  int ntap;         // Cs*R*S
  int vec;          // p is 16-byte aligned
  FastDiv dHWm, dWm, dRS, dS, dsh, dsw;
};

// source coordinate of grid coordinate g under tap offset t; false where
// the tap reads padding (forward) or no output reads this input (gx)
template <bool GX>
__device__ __forceinline__ bool src_coord(int g, int t, int stride,
                                          const FastDiv& dstride, int pad,
                                          int lim, int& v) {
  if (!GX) {
    v = g * stride - pad + t;
    return v >= 0 && v < lim;
  }
  const int tt = g + pad - t;
  if (tt < 0) return false;
  v = dstride.div(tt);
  return v * stride == tt && v < lim;
}

struct Pixel {  // a pixel index m taken apart
  int b, y, x;
};

__device__ __forceinline__ Pixel pixel_of(const ConvSrc& g, int m) {
  Pixel q;
  q.b = g.dHWm.div(m);
  const int pix = m - q.b * g.Hm * g.Wm;
  q.y = g.dWm.div(pix);
  q.x = pix - q.y * g.Wm;
  return q;
}

// 8 scattered elements: p[off[j]] where bit j of `ok` is set, zero elsewhere.
// Every load is issued, masked-out ones from element 0, and the selection
// happens afterwards: the 8 loads are independent and in flight together,
// where a load under its own branch would wait out one latency each.
__device__ __forceinline__ Chunk gather8(const bf16_t* __restrict__ p,
                                         const int64_t (&off)[8],
                                         unsigned ok) {
  bf16_t t[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) t[j] = p[(ok >> j) & 1u ? off[j] : 0];
  Chunk c;
#pragma unroll
  for (int j = 0; j < 8; ++j) c.e[j] = (ok >> j) & 1u ? t[j] : (bf16_t)0;
  return c;
}

// elements (tap kk, the `nvalid` pixels from q on, at most 8); the rest and
// invalid taps as zero
template <bool GX>
__device__ __forceinline__ Chunk conv_gather8(const ConvSrc& g, int kk,
                                              Pixel q, int nvalid) {
  Chunk c = zero_chunk();
  if (kk >= g.ntap || nvalid <= 0) return c;
  const int ch = g.dRS.div(kk), rs = kk - ch * g.R * g.S;
  const int r = g.dS.div(rs), s = rs - r * g.S;
  int sy = 0;
  bool yok = src_coord<GX>(q.y, r, g.sh, g.dsh, g.ph, g.Hs, sy);
  // first element of source row sy of plane (b, ch)
  const int64_t plane = ((int64_t)q.b * g.Cs + ch) * g.Hs;
  int64_t row = (plane + sy) * g.Ws;

  if (g.sw == 1 && q.x + 8 <= g.Wm && nvalid >= 8) {
    // 8 pixels of one grid row: 8 consecutive source columns
    if (!yok) return c;
    const int sx0 = GX ? q.x + g.pw - s : q.x - g.pw + s;
    if (sx0 >= 0 && sx0 + 8 <= g.Ws) {
      const int64_t idx = row + sx0;
      if (g.vec && (idx & 7) == 0) {
        c.raw = *reinterpret_cast<const uint4*>(g.p + idx);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) c.e[j] = g.p[idx + j];
      }
      return c;
    }
  }
  int64_t off[8];
  unsigned ok = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    int sx = 0;
    const bool v = j < nvalid && yok &&
                   src_coord<GX>(q.x, s, g.sw, g.dsw, g.pw, g.Ws, sx);
    off[j] = row + sx;
    ok |= (unsigned)v << j;
    if (++q.x == g.Wm) {  // next grid row; past the last pixel j >= nvalid
      q.x = 0;
      if (++q.y == g.Hm) { q.y = 0; ++q.b; }
      yok = src_coord<GX>(q.y, r, g.sh, g.dsh, g.ph, g.Hs, sy);
      row = ((((int64_t)q.b * g.Cs + ch) * g.Hs) + sy) * g.Ws;
    }
  }
  return gather8(g.p, off, ok);
}

// A operand of forward and gx: GEMM rows are pixels, k are taps; the chunk
// runs along the rows (transposed layout).  A thread's 8 pixels are the
// same for every K tile, so they are taken apart once, in the kernel.
template <bool GX>
struct PixelRowsLoader {
  ConvSrc g;
  Pixel q;     // this thread's first pixel, row r0 + chunk_lo(tid)
  int nvalid;  // how many of its 8 pixels are below M
  __device__ __forceinline__ PixelRowsLoader(const ConvSrc& g_, int M)
      : g(g_) {
    const int m = blockIdx.x * BM + chunk_lo(threadIdx.x);
    q = pixel_of(g, m < M ? m : 0);
    nvalid = M - m;
  }
  __device__ __forceinline__ void load(int, int k0, int kend, int tid,
                                       Chunk (&reg)[NPASS]) const {
#pragma unroll
    for (int p = 0; p < NPASS; ++p) {
      const int kk = k0 + chunk_hi(p, tid);
      reg[p] = kk < kend ? conv_gather8<GX>(g, kk, q, nvalid) : zero_chunk();
    }
  }
};

// B operand of gw: GEMM rows are taps, k are pixels; the chunk runs along
// k (plain layout)
struct TapRowsLoader {
  ConvSrc g;
  __device__ __forceinline__ void load(int r0, int k0, int kend, int tid,
                                       Chunk (&reg)[NPASS]) const {
    const int m = k0 + chunk_lo(tid);
    const Pixel q = pixel_of(g, m < kend ? m : 0);
#pragma unroll
    for (int p = 0; p < NPASS; ++p)
      reg[p] = conv_gather8<false>(g, r0 + chunk_hi(p, tid), q, kend - m);
  }
};

// B operand of gx: B(c, (k,r,s)) = w[k][c][r][s]; plain layout, runs of RS
// consecutive elements
struct WeightGxLoader {
  const bf16_t* w;
  int C, RS;
  FastDiv dRS;
  __device__ __forceinline__ void load(int r0, int k0, int kend, int tid,
                                       Chunk (&reg)[NPASS]) const {
#pragma unroll
    for (int p = 0; p < NPASS; ++p) {
      const int c = r0 + chunk_hi(p, tid);
      const int kk = k0 + chunk_lo(tid);
      Chunk v = zero_chunk();
      if (c < C && kk < kend) {
        int kq = dRS.div(kk), rs = kk - kq * RS;
        int64_t off[8];
        unsigned ok = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          off[j] = ((int64_t)kq * C + c) * RS + rs;
          ok |= (unsigned)(kk + j < kend) << j;
          if (++rs == RS) { rs = 0; ++kq; }
        }
        v = gather8(w, off, ok);
      }
      reg[p] = v;
    }
  }
};

// A operand of gw: A(k, (b,pixel)) = gy[b][k][pixel]; plain layout
struct GyRowsLoader {
  const bf16_t* gy;
  int K, OHW;
  int vec;
  FastDiv dOHW;
  __device__ __forceinline__ void load(int r0, int k0, int kend, int tid,
                                       Chunk (&reg)[NPASS]) const {
#pragma unroll
    for (int p = 0; p < NPASS; ++p) {
      const int k = r0 + chunk_hi(p, tid);
      const int q = k0 + chunk_lo(tid);
      Chunk v = zero_chunk();
      if (k < K && q < kend) {
        int b = dOHW.div(q), pix = q - b * OHW;
        if (pix + 8 <= OHW && q + 8 <= kend) {
          const int64_t idx = ((int64_t)b * K + k) * OHW + pix;
          if (vec && (idx & 7) == 0) {
            v.raw = *reinterpret_cast<const uint4*>(gy + idx);
          } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) v.e[j] = gy[idx + j];
          }
        } else {
          int64_t off[8];
          unsigned ok = 0;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            off[j] = ((int64_t)b * K + k) * OHW + pix;
            ok |= (unsigned)(q + j < kend) << j;
            if (++pix == OHW) { pix = 0; ++b; }
          }
          v = gather8(gy, off, ok);
        }
      }
      reg[p] = v;
    }
  }
};

// epilogue: GEMM row m = (b, pixel), column n = channel -> NCHW.  NCHW is
// contiguous along m, the accumulator fragments along n, so the tile goes
// through LDS (Ct[n][m]) and each thread writes 8 consecutive pixels of
// one channel: 16 bytes (bf16) or 2 x 16 bytes (fp32) where aligned.
template <typename OutT>
__device__ __forceinline__ void store8(OutT* dst, const float (&v)[8]) {
  Vec<OutT, 8> c;  // rounded once, ahead of the branch
#pragma unroll
  for (int j = 0; j < 8; ++j) from_f(v[j], c.e[j]);
  if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
    *reinterpret_cast<decltype(c.raw)*>(dst) = c.raw;
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) dst[j] = c.e[j];
  }
}

template <typename OutT>
struct NchwOut {
  static constexpr bool kTiled = true;
  OutT* out;
  int N, HW;
  FastDiv dHW;
  __device__ __forceinline__ void store_tile(const float (*Ct)[CT_LD], int m0,
                                             int n0, int M, int tid) const {
#pragma unroll
    for (int p = 0; p < NPASS; ++p) {
      const int nl = chunk_hi(p, tid), ml = chunk_lo(tid);
      const int n = n0 + nl, m = m0 + ml;
      if (n >= N || m >= M) continue;
      const float4 lo = *reinterpret_cast<const float4*>(&Ct[nl][ml]);
      const float4 hi = *reinterpret_cast<const float4*>(&Ct[nl][ml + 4]);
      const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
      int b = dHW.div(m), pix = m - b * HW;
      if (pix + 8 <= HW && m + 8 <= M) {
        store8(out + ((int64_t)b * N + n) * HW + pix, v);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (m + j < M) {
            from_f(v[j], out[((int64_t)b * N + n) * HW + pix]);
            if (++pix == HW) { pix = 0; ++b; }
          }
        }
      }
    }
  }
};

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------
template <typename OutT>
__global__ __launch_bounds__(BLK) void conv_bf16_fwd_kernel(
    ConvSrc x, Operand w, int M, OutT* __restrict__ out,
    const float* __restrict__ bias) {
  const int N = w.rows;
  gemm_bf16_block<true, false>(PixelRowsLoader<false>(x, M),
                               PlainLoader<false>{w}, M, N, x.ntap, x.ntap,
                               bias, 0, (float*)nullptr,
                               NchwOut<OutT>{out, N, x.Hm * x.Wm, x.dHWm});
}

template <typename OutT>
__global__ __launch_bounds__(BLK) void conv_bf16_bwd_x_kernel(
    ConvSrc gy, const bf16_t* __restrict__ w, int M, int C,
    OutT* __restrict__ gx) {
  gemm_bf16_block<true, false>(PixelRowsLoader<true>(gy, M),
                               WeightGxLoader{w, C, gy.R * gy.S, gy.dRS}, M,
                               C,
                               gy.ntap, gy.ntap, (const float*)nullptr, 0,
                               (float*)nullptr,
                               NchwOut<OutT>{gx, C, gy.Hm * gy.Wm, gy.dHWm});
}

__global__ __launch_bounds__(BLK) void conv_bf16_bwd_w_kernel(
    GyRowsLoader gy, ConvSrc x, int red, int kchunk, float* __restrict__ gw,
    float* __restrict__ colsum) {
  gemm_bf16_block<false, false>(gy, TapRowsLoader{x}, gy.K, x.ntap, red,
                                kchunk, (const float*)nullptr, 0, colsum,
                                RowMajorOut<float>{gw, gy.K, x.ntap});
}

// ---------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------
struct ConvDims {
  int B, C, H, W, K, R, S, sh, sw, ph, pw;
  int OH, OW;
};

// GEMM row/column/reduction counts are ints in the kernel and tile origins
// go up to one tile past them; flattened element indices are int64.
constexpr int64_t MAX_DIM = 2147483647LL - 2 * BM;

static ConvDims conv_dims(int B, int C, int H, int W, int K, int R, int S_,
                          int sh, int sw, int ph, int pw) {
  if (B < 1 || C < 1 || H < 1 || W < 1 || K < 1 || R < 1 || S_ < 1)
    throw std::invalid_argument("conv2d_bf16: every dimension must be >= 1");
  if (sh < 1 || sw < 1 || ph < 0 || pw < 0)
    throw std::invalid_argument(
        "conv2d_bf16: stride must be >= 1 and padding >= 0");
  const int64_t oh = ((int64_t)H + 2LL * ph - R) / sh + 1;
  const int64_t ow = ((int64_t)W + 2LL * pw - S_) / sw + 1;
  if ((int64_t)H + 2LL * ph < R || (int64_t)W + 2LL * pw < S_ || oh < 1 ||
      ow < 1)
    throw std::invalid_argument("conv2d_bf16: output would be empty");
  const int64_t lim[] = {
      (int64_t)B * oh * ow, (int64_t)B * H * W, (int64_t)C * R * S_,
      (int64_t)K * R * S_,  (int64_t)H + 2LL * ph, (int64_t)W + 2LL * pw,
      (int64_t)H * W,       oh * ow};
  for (int64_t v : lim)
    if (v > MAX_DIM)
      throw std::invalid_argument(
          "conv2d_bf16: a GEMM dimension does not fit the kernel's 32-bit "
          "index");
  return ConvDims{B, C, H, W, K, R, S_, sh, sw, ph, pw, (int)oh, (int)ow};
}

static ConvSrc src_x(uintptr_t x, const ConvDims& d) {  // forward, gw
  return ConvSrc{(const bf16_t*)x, d.C,  d.H,  d.W,  d.OH, d.OW,
                 d.R,              d.S,  d.sh, d.sw, d.ph, d.pw,
                 d.C * d.R * d.S,  x % 16 == 0,
                 fast_div(d.OH * d.OW), fast_div(d.OW), fast_div(d.R * d.S),
                 fast_div(d.S), fast_div(d.sh), fast_div(d.sw)};
}

static ConvSrc src_gy(uintptr_t gy, const ConvDims& d) {  // gx
  return ConvSrc{(const bf16_t*)gy, d.K,  d.OH, d.OW, d.H,  d.W,
                 d.R,               d.S,  d.sh, d.sw, d.ph, d.pw,
                 d.K * d.R * d.S,   gy % 16 == 0,
                 fast_div(d.H * d.W), fast_div(d.W), fast_div(d.R * d.S),
                 fast_div(d.S), fast_div(d.sh), fast_div(d.sw)};
}

// out[B,K,OH,OW] = conv(x[B,C,H,W], w[K,C,R,S]) (+ bias); x, w bf16
void conv2d_bf16_fwd(uintptr_t x, uintptr_t w, uintptr_t bias, uintptr_t out,
                     int B, int C, int H, int W, int K, int R, int S_, int sh,
                     int sw, int ph, int pw, bool out_f32, uintptr_t stream) {
  const ConvDims d = conv_dims(B, C, H, W, K, R, S_, sh, sw, ph, pw);
  const int M = B * d.OH * d.OW;
  const ConvSrc a = src_x(x, d);
  const Operand b = operand(w, a.ntap, K);
  const dim3 grid(cdiv(M, BM), cdiv(K, BN), 1);
  if (out_f32)
    hipLaunchKernelGGL((conv_bf16_fwd_kernel<float>), grid, dim3(BLK), 0,
                       S(stream), a, b, M, (float*)out, (const float*)bias);
  else
    hipLaunchKernelGGL((conv_bf16_fwd_kernel<bf16_t>), grid, dim3(BLK), 0,
                       S(stream), a, b, M, (bf16_t*)out, (const float*)bias);
}

// gx[B,C,H,W] from gy[B,K,OH,OW] and w; every element is written
void conv2d_bf16_bwd_x(uintptr_t gy, uintptr_t w, uintptr_t gx, int B, int C,
                       int H, int W, int K, int R, int S_, int sh, int sw,
                       int ph, int pw, bool out_f32, uintptr_t stream) {
  const ConvDims d = conv_dims(B, C, H, W, K, R, S_, sh, sw, ph, pw);
  const int M = B * H * W;
  const ConvSrc a = src_gy(gy, d);
  const dim3 grid(cdiv(M, BM), cdiv(C, BN), 1);
  if (out_f32)
    hipLaunchKernelGGL((conv_bf16_bwd_x_kernel<float>), grid, dim3(BLK), 0,
                       S(stream), a, (const bf16_t*)w, M, C, (float*)gx);
  else
    hipLaunchKernelGGL((conv_bf16_bwd_x_kernel<bf16_t>), grid, dim3(BLK), 0,
                       S(stream), a, (const bf16_t*)w, M, C, (bf16_t*)gx);
}

// how many splits of the B*OH*OW reduction the weight gradient uses
int conv2d_bf16_gw_splits(int B, int C, int H, int W, int K, int R, int S_,
                          int sh, int sw, int ph, int pw) {
  const ConvDims d = conv_dims(B, C, H, W, K, R, S_, sh, sw, ph, pw);
  return gw_split_count(B * d.OH * d.OW, K, C * R * S_);
}

// gw[K,C,R,S] (fp32), gb[K] = sum gy (fp32, 0 = skip).
// part: fp32 workspace of splits*(K*C*R*S + K) floats (unused when
// splits == 1).
void conv2d_bf16_bwd_w(uintptr_t gy, uintptr_t x, uintptr_t gw, uintptr_t gb,
                       uintptr_t part, int splits, int B, int C, int H, int W,
                       int K, int R, int S_, int sh, int sw, int ph, int pw,
                       uintptr_t stream) {
  const ConvDims d = conv_dims(B, C, H, W, K, R, S_, sh, sw, ph, pw);
  const int red = B * d.OH * d.OW, N = C * R * S_;
  if (splits != gw_split_count(red, K, N))
    throw std::invalid_argument("conv2d_bf16_bwd_w: wrong split count");
  const GyRowsLoader a{(const bf16_t*)gy, K, d.OH * d.OW, gy % 16 == 0,
                       fast_div(d.OH * d.OW)};
  const ConvSrc b = src_x(x, d);
  const int kchunk = gw_split_chunk(red, splits);
  const dim3 grid(cdiv(K, BM), cdiv(N, BN), splits);
  const int64_t n_gw = (int64_t)K * N;
  float* c = (float*)gw;
  float* cs = (float*)gb;
  if (splits > 1) {
    if (!part) throw std::invalid_argument("conv2d_bf16_bwd_w: no workspace");
    c = (float*)part;
    cs = gb ? c + (int64_t)splits * n_gw : nullptr;
  }
  hipLaunchKernelGGL(conv_bf16_bwd_w_kernel, grid, dim3(BLK), 0, S(stream), a,
                     b, red, kchunk, c, cs);
  if (splits > 1)
    hipLaunchKernelGGL(gw_combine_kernel, dim3(grid_for(n_gw, BLK)),
                       dim3(BLK), 0, S(stream), (const float*)c, (float*)gw,
                       n_gw, (const float*)cs, (float*)gb, K, splits);
}

}  // namespace

void register_conv_bf16(pybind11::module_& m) {
  m.def("conv2d_bf16_fwd", &conv2d_bf16_fwd);
  m.def("conv2d_bf16_bwd_x", &conv2d_bf16_bwd_x);
  m.def("conv2d_bf16_gw_splits", &conv2d_bf16_gw_splits);
  m.def("conv2d_bf16_bwd_w", &conv2d_bf16_bwd_w);
}
