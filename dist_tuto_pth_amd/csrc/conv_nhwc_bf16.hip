// K17, channels-last — bf16 convolution on the CDNA4 matrix cores (gfx950)
// for tensors stored [B][H][W][C] (torch.channels_last).
//
// Numeric contract is conv_bf16.hip's (ops.conv2d_bf16): bf16 operands,
// fp32 accumulation on v_mfma_f32_16x16x32_bf16, ONE rounding (RNE) per
// result, padding contributes exact zeros, gw/gb in fp32 without float
// atomics and bitwise reproducible.
//
// Three implicit GEMMs on 64x64x64 tiles, 2x2 waves.  The reduction index
// is always channel-fastest, so 8 consecutive reduction elements of one
// pixel are 8 consecutive addresses whatever the stride, the filter column
// or the distance to the image edge:
//
//   product   rows M     cols N     reduction       A                B
//   forward   B*OH*OW    K          (r,s,c)         x gathered       packed w
//   gx        B*H*W      C          (r,s,k)         gy gathered      packed w'
//   gw (+gb)  K          (r,s,c)    B*OH*OW, split  gy (T)           x gathered (T)
//
// packed w is [K][R][S][C], packed w' is [C][R][S][K]; both are written
// from the master weight ([K,C,R,S], fp32 or bf16) by pack_weight_kernel,
// which is also the weight's one rounding to bf16.
//
// Forward and gx run a block loop of their own (conv_nhwc_kernel), because
// their A loader carries state across K tiles: a thread's two pixels are
// taken apart once, the tap (r,s) and the channel offset then advance by
// additions.  With Cs % 8 == 0 a chunk is one 16-byte load, issued from a
// safe address and zeroed afterwards where the tap reads padding; it goes
// to LDS with one 16-byte write.  Any other Cs takes a per-element path
// whose chunks may straddle taps.  GEMM row (b, pixel) by column channel is
// the output's own row-major order: the epilogue rounds each result once,
// stages the OutT tile in the operand LDS, which is free by then, and every
// thread writes 8 consecutive channels.  LDS per block is the two operand
// tiles, 18432 bytes, as in linear_bf16.
//
// Forward with a statistics epilogue (conv_nhwc_stats_kernel, STATS = true;
// ops.conv2d_bf16(..., bn_stats=True)).  Besides storing its tile, the block
// reduces the live rows (m < M) of the staged OutT tile, i.e. the stored
// values after their one rounding, bias included, to a per-channel mean and
// centred second moment M2 = sum (v - mean)^2 in fp32, and writes them to
// tws[row tile][N][2] with one 8-byte store per channel.  The count is not
// stored: it is min(BM, M - m0).  Split of the 64x64 tile over the 256
// threads: wave q owns rows [16q, 16q+16), lane c owns tile column c, so an
// LDS read of a row is 64 adjacent elements and hits every bank once.  A
// thread reads its 16 values once, keeps them in the registers the
// accumulators have left, and adds the live ones in ascending row order;
// the four waves' sums go through 4x64 floats of LDS and every thread adds
// them in wave order 0..3 and divides by the count, so the four threads of
// a channel hold the same mean.  The second pass runs over the same 16
// values: d = v - mean, fmaf(d, d, .) in ascending row order, the four
// partial M2 again added in wave order by thread c of wave 0.  Every sum's
// order is fixed by (M, N) alone, whatever the load path (VEC) or the
// alignment; there are no atomics.  The 1,024 bytes of scratch are the ones
// the fp32 C tile leaves free in the operand tiles (the bf16 tile leaves
// more), so LDS stays at 18,432 bytes.  The global stores of the tile are
// issued before the reduction and fly under it.  STATS is a template flag:
// the kernels without it are the ones they were.
//
// gw runs on gemm_bf16_block with both operands transposed on the LDS
// write (the reduction runs along pixels, the chunks along channels).  Its
// epilogue stores column (r,s,c) at the parameter's [K,C,R,S] position, so
// the split partials and gw_combine_kernel work on the dense layout.
//
// Bindings are registered from kernels.hip's PYBIND11_MODULE through
// register_conv_nhwc_bf16().

#include "gemm_bf16.h"

#include <pybind11/pybind11.h>

namespace {

// ---------------------------------------------------------------------------
// the gather
// ---------------------------------------------------------------------------
// A pixel index m runs over (b, y, x) of a grid Hm x Wm; a reduction index
// kk runs over (r, s, ch) with ch fastest.  Forward and gw read x at
// (y*sh - ph + r, x*sw - pw + s), the grid being the OUTPUT plane.  gx reads
// gy at ((y + ph - r)/sh, (x + pw - s)/sw) where those divide exactly, the
// grid being the INPUT plane.
struct NhwcSrc {
  const bf16_t* p;  // [B, Hs, Ws, Cs]
  int Cs, Hs, Ws;
  int Hm, Wm;       // pixel grid
  int R, S, sh, sw, ph, pw;
  int nred;         // R*S*Cs
  int step_c, step_s;  // BK = step_s*Cs + step_c: one K tile, in taps
  FastDiv dHWm, dWm, dCs, dS, dsh, dsw;
};

struct Tap {  // a reduction index taken apart
  int r, s, c;
};

__device__ __forceinline__ Tap tap_of(const NhwcSrc& g, int kk) {
  Tap t;
  const int rs = g.dCs.div(kk);
  t.c = kk - rs * g.Cs;
  t.r = g.dS.div(rs);
  t.s = rs - t.r * g.S;
  return t;
}

// one element further along the reduction
__device__ __forceinline__ void tap_inc(const NhwcSrc& g, Tap& t) {
  if (++t.c == g.Cs) {
    t.c = 0;
    if (++t.s == g.S) { t.s = 0; ++t.r; }
  }
}

// one K tile (BK elements) further, without a division.  The loop runs
// BK / (Cs * S) times, rounded up: at most once where Cs * S >= BK, up to
// BK times for a one-channel, one-column filter (per-element path only).
__device__ __forceinline__ void tap_next_tile(const NhwcSrc& g, Tap& t) {
  t.c += g.step_c;
  t.s += g.step_s;
  if (t.c >= g.Cs) { t.c -= g.Cs; ++t.s; }
  while (t.s >= g.S) { t.s -= g.S; ++t.r; }
}

// gx: the output coordinate that reads input coordinate tt - pad under this
// tap, where one exists (conv_bf16.hip's src_coord<true>, branch-free)
__device__ __forceinline__ bool strided_src(int tt, int stride,
                                            const FastDiv& dstride, int lim,
                                            int& v) {
  v = dstride.div(tt < 0 ? 0 : tt);
  return tt >= 0 && v * stride == tt && v < lim;
}

// A pixel's fixed part, taken apart once.  Forward/gw: (y0, x0) is the
// window's corner y*sh - ph, x*sw - pw and pb the pixel index of that
// corner in the source, (b*Hs + y0)*Ws + x0.  gx: (y0, x0) is y + ph,
// x + pw and pb = b*Hs.  Pixel indices are computed modulo 2^32: the index
// of an element that exists is below 2^31 and comes out exact, one of
// padding is never used.
struct Window {
  uint32_t pb;
  int y0, x0;
};

template <bool GX>
__device__ __forceinline__ Window window_of(const NhwcSrc& g, int m) {
  const int b = g.dHWm.div(m);
  const int pix = m - b * g.Hm * g.Wm;
  const int y = g.dWm.div(pix), x = pix - y * g.Wm;
  Window w;
  if (GX) {
    w.y0 = y + g.ph;
    w.x0 = x + g.pw;
    w.pb = (uint32_t)b * g.Hs;
  } else {
    w.y0 = y * g.sh - g.ph;
    w.x0 = x * g.sw - g.pw;
    w.pb = ((uint32_t)b * g.Hs + w.y0) * g.Ws + w.x0;
  }
  return w;
}

// element offset of (window, tap) in the source; false where the tap reads
// padding (forward, gw) or no output reads this input under it (gx).  The
// offset is only meaningful where the result is true.
template <bool GX>
__device__ __forceinline__ bool src_at(const NhwcSrc& g, const Window& w,
                                       const Tap& u, int64_t& off) {
  if (!GX) {
    const int sy = w.y0 + u.r, sx = w.x0 + u.s;
    off = (int64_t)(w.pb + (uint32_t)u.r * g.Ws + u.s) * g.Cs + u.c;
    return (unsigned)sy < (unsigned)g.Hs && (unsigned)sx < (unsigned)g.Ws;
  }
  int sy, sx;
  const bool yok = strided_src(w.y0 - u.r, g.sh, g.dsh, g.Hs, sy);
  const bool xok = strided_src(w.x0 - u.s, g.sw, g.dsw, g.Ws, sx);
  off = (int64_t)((w.pb + sy) * g.Ws + sx) * g.Cs + u.c;
  return yok && xok;
}

// The 8 reduction elements from kk (= tap t) of one window; elements at or
// past nred, and all of them where !live, are zero.  Every load is issued,
// masked-out ones from element 0, and the selection happens afterwards, so
// that a thread's loads are in flight together.
// VEC (Cs % 8 == 0, p 16-byte aligned, kk % 8 == 0): the chunk lies in one
// tap and is one aligned 16-byte load.
template <bool GX, bool VEC>
__device__ __forceinline__ Chunk fetch8(const NhwcSrc& g, const Window& w,
                                        bool live, int kk, Tap t) {
  Chunk c;
  if (VEC) {
    int64_t off;
    const bool ok = src_at<GX>(g, w, t, off) && live && kk < g.nred;
    c.raw = *reinterpret_cast<const uint4*>(g.p + (ok ? off : 0));
    if (!ok) c = zero_chunk();
    return c;
  }
  bf16_t v[8];
  unsigned ok = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    int64_t off;
    const bool e = src_at<GX>(g, w, t, off) && live && kk + j < g.nred;
    v[j] = g.p[e ? off : 0];
    ok |= (unsigned)e << j;
    tap_inc(g, t);
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) c.e[j] = (ok >> j) & 1u ? v[j] : (bf16_t)0;
  return c;
}

// A operand of forward and gx: GEMM rows are pixels, k is the reduction
// index; the chunk runs along k (plain layout).  A thread owns the same
// NPASS rows and the same chunk column in every K tile.
template <bool GX, bool VEC>
struct PixelLoader {
  const NhwcSrc& g;
  Window w[NPASS];
  bool live[NPASS];  // row below M
  int kk;            // reduction index of this thread's next chunk
  Tap t;
  __device__ __forceinline__ PixelLoader(const NhwcSrc& g_, int m0, int M,
                                         int tid)
      : g(g_) {
#pragma unroll
    for (int p = 0; p < NPASS; ++p) {
      const int m = m0 + chunk_hi(p, tid);
      live[p] = m < M;
      w[p] = window_of<GX>(g, live[p] ? m : 0);
    }
    kk = chunk_lo(tid);
    t = tap_of(g, kk);
  }
  // this thread's chunks of the current K tile; then on to the next tile
  __device__ __forceinline__ void load(Chunk (&reg)[NPASS]) {
#pragma unroll
    for (int p = 0; p < NPASS; ++p)
      reg[p] = fetch8<GX, VEC>(g, w[p], live[p], kk, t);
    kk += BK;
    tap_next_tile(g, t);
  }
};

// B operand of gw: GEMM rows are columns n = (r,s,c) of the weight
// gradient, k are output pixels; the chunk runs along the rows
// (transposed layout).  A thread's 8 columns are the same for every K
// tile, its pixels change.
template <bool VEC>
struct TapColsLoader {
  NhwcSrc g;
  int n;  // first of this thread's 8 columns
  Tap t;
  __device__ __forceinline__ TapColsLoader(const NhwcSrc& g_) : g(g_) {
    n = blockIdx.y * BN + chunk_lo(threadIdx.x);
    t = tap_of(g, n);
  }
  __device__ __forceinline__ void load(int, int k0, int kend, int tid,
                                       Chunk (&reg)[NPASS]) const {
#pragma unroll
    for (int p = 0; p < NPASS; ++p) {
      const int m = k0 + chunk_hi(p, tid);
      const bool live = m < kend;
      reg[p] = fetch8<false, VEC>(g, window_of<false>(g, live ? m : 0), live,
                                  n, t);
    }
  }
};

// epilogue of gw: GEMM column n = (r,s,c) goes to the parameter's
// [K][C][R][S] position, in the result or in split z's partial
struct GwOut {
  static constexpr bool kTiled = false;
  float* gw;
  int K, C, RS;
  FastDiv dC;
  __device__ __forceinline__ void operator()(int z, int m, int n,
                                             float v) const {
    const int rs = dC.div(n), c = n - rs * C;
    gw[(((int64_t)z * K + m) * C + c) * RS + rs] = v;
  }
};

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------
constexpr int OPER_BYTES = (BM + BN) * LDS_LD * (int)sizeof(bf16_t);

// out[m][n] = bias[n] + sum_kk A(m,kk) * w[n][kk], rounded once to OutT;
// out is row-major [M][N].  grid = (m tiles, n tiles).
// STATS: also tws[blockIdx.x][n][0..1] = (mean, M2) of the block's live
// rows of column n, from the staged (stored) values.
template <bool GX, bool VEC, typename OutT, bool STATS>
__device__ __forceinline__ void conv_nhwc_block(
    NhwcSrc a, Operand w, int M, int N, OutT* __restrict__ out,
    const float* __restrict__ bias, int out_vec, float* __restrict__ tws) {
  // the C tile's pitch keeps rows 16-byte aligned and off a common bank
  constexpr int CT_PITCH = BN + 16 / (int)sizeof(OutT);
  static_assert(BM * CT_PITCH * sizeof(OutT) <= OPER_BYTES,
                "the C tile is staged in the operand tiles");
  __shared__ __attribute__((aligned(16))) unsigned char smem[OPER_BYTES];
  bf16_t (*As)[LDS_LD] = reinterpret_cast<bf16_t(*)[LDS_LD]>(smem);
  bf16_t (*Bs)[LDS_LD] = As + BM;
  OutT (*Ct)[CT_PITCH] = reinterpret_cast<OutT(*)[CT_PITCH]>(smem);

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const int kend = a.nred;

  // a fragment holds 4 consecutive m of one n, so the accumulators start
  // from that column's bias and the epilogue only converts
  frag_cd acc[2][2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = n0 + wn + j * 16 + (lane & 15);
    const float bv = (bias && n < N) ? bias[n] : 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) acc[i][j] = frag_cd{bv, bv, bv, bv};
  }

  PixelLoader<GX, VEC> A(a, m0, M, tid);
  Chunk ra[NPASS], rb[NPASS];
  A.load(ra);
  gload<false>(w, n0, 0, kend, tid, rb);
  for (int k0 = 0; k0 < kend; k0 += BK) {
    lds_store<false>(As, tid, ra);
    lds_store<false>(Bs, tid, rb);
    __syncthreads();
    if (k0 + BK < kend) {  // next tile's global loads fly under the MFMAs
      A.load(ra);
      gload<false>(w, n0, k0 + BK, kend, tid, rb);
    }
#pragma unroll
    for (int ks = 0; ks < BK; ks += 32) {
      const int kk = ks + 8 * (lane >> 4);
      frag_ab fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int ar = wm + i * 16 + (lane & 15);
        const int br = wn + i * 16 + (lane & 15);
        fa[i] = *reinterpret_cast<const frag_ab*>(&As[ar][lds_col(ar, kk)]);
        fb[i] = *reinterpret_cast<const frag_ab*>(&Bs[br][lds_col(br, kk)]);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();  // also frees the operand tiles for the C tile
  }

  // round once, stage as OutT
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int nl = wn + j * 16 + (lane & 15);
      const int ml = wm + i * 16 + (lane >> 4) * 4;
#pragma unroll
      for (int r = 0; r < 4; ++r) from_f(acc[i][j][r], Ct[ml + r][nl]);
    }
  __syncthreads();
  // each thread writes 8 consecutive channels of NPASS pixels
#pragma unroll
  for (int p = 0; p < NPASS; ++p) {
    const int ml = chunk_hi(p, tid), nl = chunk_lo(tid);
    const int m = m0 + ml, n = n0 + nl;
    if (m >= M || n >= N) continue;
    OutT* dst = out + (int64_t)m * N + n;
    if (out_vec) {  // N % 8 == 0: the run is whole and aligned
      using RawT = decltype(Vec<OutT, 8>::raw);
      *reinterpret_cast<RawT*>(dst) =
          *reinterpret_cast<const RawT*>(&Ct[ml][nl]);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (n + j < N) dst[j] = Ct[ml][nl + j];
    }
  }

  if constexpr (STATS) {
    static_assert(BN == 64 && BM % NWAVE == 0, "a lane per column");
    constexpr int SEG = BM / NWAVE;  // rows per wave
    constexpr int RED_OFF = OPER_BYTES - NWAVE * BN * (int)sizeof(float);
    static_assert(BM * CT_PITCH * sizeof(OutT) <= RED_OFF,
                  "the wave sums lie behind the C tile");
    float (*red)[BN] = reinterpret_cast<float(*)[BN]>(smem + RED_OFF);
    const int live = min(BM, M - m0);  // rows of this tile, >= 1
    const int nrow = min(SEG, live - wave * SEG);  // of this wave, may be <= 0
    float v[SEG];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < SEG; ++i) {
      v[i] = to_f(Ct[wave * SEG + i][lane]);
      if (i < nrow) s += v[i];
    }
    red[wave][lane] = s;
    __syncthreads();
    const float mean =
        (((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane]) /
        (float)live;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < SEG; ++i)
      if (i < nrow) {
        const float d = v[i] - mean;
        q = fmaf(d, d, q);
      }
    __syncthreads();  // every thread has read the sums
    red[wave][lane] = q;
    __syncthreads();
    if (wave == 0 && n0 + lane < N) {
      const float m2 =
          ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
      *reinterpret_cast<float2*>(
          tws + ((int64_t)blockIdx.x * N + n0 + lane) * 2) =
          make_float2(mean, m2);
    }
  }
}

template <bool GX, bool VEC, typename OutT>
__global__ __launch_bounds__(BLK) void conv_nhwc_kernel(
    NhwcSrc a, Operand w, int M, int N, OutT* __restrict__ out,
    const float* __restrict__ bias, int out_vec) {
  conv_nhwc_block<GX, VEC, OutT, false>(a, w, M, N, out, bias, out_vec,
                                        nullptr);
}

// the forward with the statistics epilogue
template <bool VEC, typename OutT>
__global__ __launch_bounds__(BLK) void conv_nhwc_stats_kernel(
    NhwcSrc a, Operand w, int M, int N, OutT* __restrict__ out,
    const float* __restrict__ bias, int out_vec, float* __restrict__ tws) {
  conv_nhwc_block<false, VEC, OutT, true>(a, w, M, N, out, bias, out_vec,
                                          tws);
}

// gw[k][(r,s,c)] = sum over pixels gy[pixel][k] * x[window(pixel)][r][s][c];
// grid = (k tiles, column tiles, splits)
template <bool VEC>
__global__ __launch_bounds__(BLK) void conv_nhwc_bwd_w_kernel(
    Operand gy, NhwcSrc x, int red, int kchunk, GwOut gw,
    float* __restrict__ colsum) {
  gemm_bf16_block<true, true>(PlainLoader<true>{gy}, TapColsLoader<VEC>(x),
                              gy.rows, x.nred, red, kchunk,
                              (const float*)nullptr, 0, colsum, gw);
}

// master weight [K][C][RS] (fp32 or bf16) -> bf16 [K][RS][C] (forward, gw)
// or [C][RS][K] (GX); the fp32 weight's one rounding
template <typename InT, bool GX>
__global__ __launch_bounds__(BLK) void pack_weight_kernel(
    const InT* __restrict__ w, bf16_t* __restrict__ out, int K, int C, int RS,
    int64_t n) {
  const int inner = GX ? K : C;
  for (int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * BLK) {
    const int64_t t = i / inner;
    const int in = (int)(i - t * inner);
    const int64_t o = t / RS;
    const int rs = (int)(t - o * RS);
    const int64_t k = GX ? in : o, c = GX ? o : in;
    from_f(to_f(w[(k * C + c) * RS + rs]), out[i]);
  }
}

// ---------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------
static NhwcSrc make_src(uintptr_t p, int Cs, int Hs, int Ws, int Hm, int Wm,
                        const ConvDims& d) {
  return NhwcSrc{(const bf16_t*)p, Cs, Hs, Ws, Hm, Wm,
                 d.R, d.S, d.sh, d.sw, d.ph, d.pw,
                 d.R * d.S * Cs, BK % Cs, BK / Cs,
                 fast_div(Hm * Wm), fast_div(Wm), fast_div(Cs), fast_div(d.S),
                 fast_div(d.sh), fast_div(d.sw)};
}
static NhwcSrc src_x(uintptr_t x, const ConvDims& d) {  // forward, gw
  return make_src(x, d.C, d.H, d.W, d.OH, d.OW, d);
}
static NhwcSrc src_gy(uintptr_t gy, const ConvDims& d) {  // gx
  return make_src(gy, d.K, d.OH, d.OW, d.H, d.W, d);
}
static bool chunks_are_vectors(const NhwcSrc& s) {
  return s.Cs % 8 == 0 && reinterpret_cast<uintptr_t>(s.p) % 16 == 0;
}

// out[M][N] from the gathered `a` and the packed weight wp[N][a.nred];
// with tws (forward only) through the statistics epilogue
template <bool GX>
static void launch_pixels(const NhwcSrc& a, uintptr_t wp, uintptr_t bias,
                          uintptr_t out, int M, int N, bool out_f32,
                          uintptr_t stream, uintptr_t tws = 0) {
  const Operand b = operand(wp, a.nred, N);
  const dim3 grid(cdiv(M, BM), cdiv(N, BN), 1);
  const int out_vec = N % 8 == 0 && out % 16 == 0;
  const bool vec = chunks_are_vectors(a);
  by_dtype(!out_f32, [&](auto* t) {
    using OutT = elem_t<decltype(t)>;
    if constexpr (!GX) {
      if (tws) {
        if (vec)
          hipLaunchKernelGGL((conv_nhwc_stats_kernel<true, OutT>), grid,
                             dim3(BLK), 0, S(stream), a, b, M, N, (OutT*)out,
                             (const float*)bias, out_vec, (float*)tws);
        else
          hipLaunchKernelGGL((conv_nhwc_stats_kernel<false, OutT>), grid,
                             dim3(BLK), 0, S(stream), a, b, M, N, (OutT*)out,
                             (const float*)bias, out_vec, (float*)tws);
        return;
      }
    }
    if (vec)
      hipLaunchKernelGGL((conv_nhwc_kernel<GX, true, OutT>), grid, dim3(BLK),
                         0, S(stream), a, b, M, N, (OutT*)out,
                         (const float*)bias, out_vec);
    else
      hipLaunchKernelGGL((conv_nhwc_kernel<GX, false, OutT>), grid, dim3(BLK),
                         0, S(stream), a, b, M, N, (OutT*)out,
                         (const float*)bias, out_vec);
  });
}

// out: bf16 [K][R][S][C], or [C][R][S][K] with for_gx, from w [K,C,R,S]
void conv2d_nhwc_bf16_pack_w(uintptr_t w, uintptr_t out, int K, int C, int R,
                             int S_, bool w_f32, bool for_gx,
                             uintptr_t stream) {
  if (K < 1 || C < 1 || R < 1 || S_ < 1 || (int64_t)R * S_ > MAX_DIM)
    throw std::invalid_argument("conv2d_bf16: bad weight shape");
  const int64_t n = (int64_t)K * C * R * S_;
  const dim3 grid(grid_for(n, BLK));
  by_dtype(!w_f32, [&](auto* t) {
    using InT = elem_t<decltype(t)>;
    if (for_gx)
      hipLaunchKernelGGL((pack_weight_kernel<InT, true>), grid, dim3(BLK), 0,
                         S(stream), (const InT*)w, (bf16_t*)out, K, C, R * S_,
                         n);
    else
      hipLaunchKernelGGL((pack_weight_kernel<InT, false>), grid, dim3(BLK), 0,
                         S(stream), (const InT*)w, (bf16_t*)out, K, C, R * S_,
                         n);
  });
}

// out[B,OH,OW,K] = conv(x[B,H,W,C], wp[K][R][S][C]) (+ bias)
void conv2d_nhwc_bf16_fwd(uintptr_t x, uintptr_t wp, uintptr_t bias,
                          uintptr_t out, int B, int C, int H, int W, int K,
                          int R, int S_, int sh, int sw, int ph, int pw,
                          bool out_f32, uintptr_t stream) {
  const ConvDims d = conv_dims(B, C, H, W, K, R, S_, sh, sw, ph, pw);
  launch_pixels<false>(src_x(x, d), wp, bias, out, B * d.OH * d.OW, K,
                       out_f32, stream);
}

// The same, and tws[tiles][K][2] = (mean, M2) over the rows
// [t*BM, min(B*OH*OW, (t+1)*BM)) of every output channel, taken from the
// stored values; tiles = conv2d_nhwc_bf16_stats_tiles(B*OH*OW).  Every
// element of tws is written.
void conv2d_nhwc_bf16_fwd_stats(uintptr_t x, uintptr_t wp, uintptr_t bias,
                                uintptr_t out, uintptr_t tws, int B, int C,
                                int H, int W, int K, int R, int S_, int sh,
                                int sw, int ph, int pw, bool out_f32,
                                uintptr_t stream) {
  if (!tws || tws % 8)
    throw std::invalid_argument(
        "conv2d_nhwc_bf16_fwd_stats: tws must be an 8-byte aligned buffer");
  const ConvDims d = conv_dims(B, C, H, W, K, R, S_, sh, sw, ph, pw);
  launch_pixels<false>(src_x(x, d), wp, bias, out, B * d.OH * d.OW, K,
                       out_f32, stream, tws);
}

int64_t conv2d_nhwc_bf16_stats_tiles(int64_t rows) {
  static_assert(BM == BN_PARTIAL_ROWS, "batch norm derives the counts");
  if (rows < 1 || rows > MAX_DIM)
    throw std::invalid_argument("conv2d_bf16: bad row count");
  return (rows + BM - 1) / BM;
}

// gx[B,H,W,C] from gy[B,OH,OW,K] and wp[C][R][S][K]; every element is
// written
void conv2d_nhwc_bf16_bwd_x(uintptr_t gy, uintptr_t wp, uintptr_t gx, int B,
                            int C, int H, int W, int K, int R, int S_, int sh,
                            int sw, int ph, int pw, bool out_f32,
                            uintptr_t stream) {
  const ConvDims d = conv_dims(B, C, H, W, K, R, S_, sh, sw, ph, pw);
  launch_pixels<true>(src_gy(gy, d), wp, 0, gx, B * H * W, C, out_f32,
                      stream);
}

// how many splits of the B*OH*OW reduction the weight gradient uses
int conv2d_nhwc_bf16_gw_splits(int B, int C, int H, int W, int K, int R,
                               int S_, int sh, int sw, int ph, int pw) {
  const ConvDims d = conv_dims(B, C, H, W, K, R, S_, sh, sw, ph, pw);
  return gw_split_count(B * d.OH * d.OW, K, C * R * S_);
}

// gw[K,C,R,S] (fp32, dense), gb[K] = sum gy (fp32, 0 = skip) from
// gy[B,OH,OW,K] and x[B,H,W,C].  part: fp32 workspace of
// splits*(K*C*R*S + K) floats (unused when splits == 1).
void conv2d_nhwc_bf16_bwd_w(uintptr_t gy, uintptr_t x, uintptr_t gw,
                            uintptr_t gb, uintptr_t part, int splits, int B,
                            int C, int H, int W, int K, int R, int S_, int sh,
                            int sw, int ph, int pw, uintptr_t stream) {
  const ConvDims d = conv_dims(B, C, H, W, K, R, S_, sh, sw, ph, pw);
  const int red = B * d.OH * d.OW, N = C * R * S_;
  if (splits != gw_split_count(red, K, N))
    throw std::invalid_argument("conv2d_nhwc_bf16_bwd_w: wrong split count");
  // A(k, pixel) = gy[pixel][k]: a transposed plain operand
  const Operand a = operand(gy, K, K);
  const NhwcSrc b = src_x(x, d);
  const int kchunk = gw_split_chunk(red, splits);
  const dim3 grid(cdiv(K, BM), cdiv(N, BN), splits);
  const int64_t n_gw = (int64_t)K * N;
  float* c = (float*)gw;
  float* cs = (float*)gb;
  if (splits > 1) {
    if (!part)
      throw std::invalid_argument("conv2d_nhwc_bf16_bwd_w: no workspace");
    c = (float*)part;
    cs = gb ? c + (int64_t)splits * n_gw : nullptr;
  }
  const GwOut epi{c, K, C, R * S_, fast_div(C)};
  if (chunks_are_vectors(b))
    hipLaunchKernelGGL(conv_nhwc_bwd_w_kernel<true>, grid, dim3(BLK), 0,
                       S(stream), a, b, red, kchunk, epi, cs);
  else
    hipLaunchKernelGGL(conv_nhwc_bwd_w_kernel<false>, grid, dim3(BLK), 0,
                       S(stream), a, b, red, kchunk, epi, cs);
  if (splits > 1)
    hipLaunchKernelGGL(gw_combine_kernel, dim3(grid_for(n_gw, BLK)),
                       dim3(BLK), 0, S(stream), (const float*)c, (float*)gw,
                       n_gw, (const float*)cs, (float*)gb, K, splits);
}

}  // namespace

void register_conv_nhwc_bf16(pybind11::module_& m) {
  m.def("conv2d_nhwc_bf16_pack_w", &conv2d_nhwc_bf16_pack_w);
  m.def("conv2d_nhwc_bf16_fwd", &conv2d_nhwc_bf16_fwd);
  m.def("conv2d_nhwc_bf16_fwd_stats", &conv2d_nhwc_bf16_fwd_stats);
  m.def("conv2d_nhwc_bf16_stats_tiles", &conv2d_nhwc_bf16_stats_tiles);
  m.def("conv2d_nhwc_bf16_bwd_x", &conv2d_nhwc_bf16_bwd_x);
  m.def("conv2d_nhwc_bf16_gw_splits", &conv2d_nhwc_bf16_gw_splits);
  m.def("conv2d_nhwc_bf16_bwd_w", &conv2d_nhwc_bf16_bwd_w);
}
