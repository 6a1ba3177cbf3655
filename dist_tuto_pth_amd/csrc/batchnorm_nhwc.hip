// batchnorm_nhwc.hip — K18 on channels-last storage: batch normalization
// over [B][H][W][C] tensors (fp32 or bf16) with the optional fused residual
// add and ReLU, forward and backward.  The contract is batchnorm.hip's:
// fp32 statistics and arithmetic, centred variance, one rounding per
// element, no float atomics, bitwise reproducible.
//
// The tensor is a matrix of rows = B*H*W by C and every kernel uses the
// tiling of nhwc_tile.h: a thread owns V adjacent channels (16, 8, 4 or 2
// bytes, the widest for which C % V == 0 and every pointer is aligned, else
// one element), CL column lanes make a tile row of CT = CL*V channels, the
// other RL = BLK/CL threads are row lanes.  CL is 16 (RL 16) from C = 128
// and 8 (RL 32) below it, so a full-width tile row is 256 or 128 bytes and
// C = 64 still is one (bf16) or two (fp32) full tiles.  Unlike an NCHW
// plane, a row is contiguous in C whatever H*W is: 14x14 and 7x7 maps move
// 16 bytes per lane like every other.
//
// Kernels:
//   bn_nhwc_stats_kernel       grid (column tiles, S): block (t, s) reduces
//                              rows [s*per, min(rows, (s+1)*per)) of its
//                              channels to (count, mean, M2) in ws[C][S][3]:
//                              the slice mean first, then the centred second
//                              moment in a second, L2-resident pass
//   bn_nhwc_merge_kernel       the statistics from the partials (mean, M2)
//                              per 64-row tile that the convolution which
//                              produced x wrote in its epilogue
//                              (conv_nhwc_bf16.hip), instead of the stats
//                              and finalize kernels: see below
//   bn_nhwc_apply_kernel       y = relu?((x-mean)*(gamma*invstd)+beta (+res))
//   bn_nhwc_bwd_reduce_kernel  grid (column tiles, S): partial dbeta /
//                              dgamma, ws[C][S][2]
//   bn_nhwc_bwd_apply_kernel   gx and/or g_residual in one pass
//   The partials are merged by bn_shared.h's finalize kernels, unchanged.
//
// Reduction order.  Within a slice, row r (counted from the slice's first)
// belongs to row lane r % RL, which adds its rows in ascending order into
// one fp32 accumulator per channel; the RL lanes of a channel are added
// through LDS in lane order (lane_combine).  Channels never mix and RL
// depends on C alone, so every sum is fixed by (rows, C, S) and not by V,
// the alignment or the dtype: the bf16 result is the fp32 one on the same
// values rounded once, and a misaligned view gives the bits of its clone.
//
// Merge order of bn_nhwc_merge_kernel.  T = ceil(rows/64) partials per
// channel, partial t covering rows [64t, min(rows, 64t+64)), are merged
// with Chan's formula on levels of 256: at a level with P partials of
// `span` rows each, group g = partials [256g, min(P, 256g+256)); in it
// tile lane l (of 16) merges partials 256g + l, + 16, + 32, ... in
// ascending order, at most 16 of them, then the 16 lanes are merged in
// lane order through LDS.  The groups' results are the next level's
// partials, span*256 rows each, until one group is left.  A thread's serial
// chain is at most 16 + 15 merges per level whatever T is; the number of
// levels is ceil(log256 T): 1 up to 16,384 rows, 2 up to 4,194,304.  Counts
// are never stored, every level derives them from (rows, span).  The order
// depends on (rows, C) only (C: which block holds a channel, not the
// order).  Adjacent threads read adjacent channels: 16 x 8 bytes per lane.
//
// The apply kernels load mean, gamma*invstd, beta (and dbeta/n, dgamma/n)
// of their V channels once into registers and then stride over rows; the
// arithmetic per element is batchnorm.hip's in the same order.
//
// Bindings are registered from kernels.hip's PYBIND11_MODULE through
// register_batchnorm_nhwc().

#include "bn_shared.h"
#include "nhwc_tile.h"

#include <pybind11/pybind11.h>

#include <algorithm>

namespace {

// fn(r) for the rows r = first, first + step, ... below end, in that order
template <int UNROLL, class F>
__device__ __forceinline__ void for_rows(uint32_t first, uint32_t end,
                                         uint32_t step, F&& fn) {
#pragma unroll UNROLL
  for (uint32_t r = first; r < end; r += step) fn(r);
}

// ---------------------------------------------------------------------------
// forward statistics
// ---------------------------------------------------------------------------
template <typename T, int V>
__global__ __launch_bounds__(BLK) void bn_nhwc_stats_kernel(
    const T* __restrict__ x, float* __restrict__ ws, uint32_t rows,
    uint32_t C, uint32_t per, int cl_shift) {
  __shared__ float sh[BLK * V];
  const ColTile t = col_tile<V>(blockIdx.x, cl_shift, C);
  const uint32_t RL = (uint32_t)BLK >> cl_shift;
  const uint32_t r0 = blockIdx.y * per, r1 = min(rows, r0 + per);
  const T* xp = x + t.c;

  float acc[V];
#pragma unroll
  for (int j = 0; j < V; ++j) acc[j] = 0.f;
  if (t.live)
    for_rows<8>(r0 + t.rl, r1, RL, [&](uint32_t r) {
      float f[V];
      load_vec<T, V>(xp + r * C, f);
#pragma unroll
      for (int j = 0; j < V; ++j) acc[j] += f[j];
    });
  const float cnt = (float)(r1 - r0);
  const float mean = lane_combine<V>(acc, t, cl_shift, sh) / cnt;
  float mu[V];
  lane_broadcast<V>(mean, t, cl_shift, sh, mu);

  // second pass over the slice (L2-resident): centred second moment
#pragma unroll
  for (int j = 0; j < V; ++j) acc[j] = 0.f;
  if (t.live)
    for_rows<8>(r0 + t.rl, r1, RL, [&](uint32_t r) {
      float f[V];
      load_vec<T, V>(xp + r * C, f);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float d = f[j] - mu[j];
        acc[j] = fmaf(d, d, acc[j]);
      }
    });
  const float m2 = lane_combine<V>(acc, t, cl_shift, sh);
  const uint32_t c = (blockIdx.x << cl_shift) * V + threadIdx.x;
  if (threadIdx.x < ((uint32_t)V << cl_shift) && c < C) {
    float* o = ws + ((int64_t)c * gridDim.y + blockIdx.y) * 3;
    o[0] = cnt;
    o[1] = mean;
    o[2] = m2;
  }
}

// ---------------------------------------------------------------------------
// forward statistics from the convolution's partials
// ---------------------------------------------------------------------------
// Chan's merge of (na, mean, m2) with (nb, mb, m2b), nb > 0: the arithmetic
// of bn_finalize_kernel
__device__ __forceinline__ void chan_merge(float& n, float& mean, float& m2,
                                           float nb, float mb, float m2b) {
  const float nab = n + nb, delta = mb - mean;
  mean += delta * (nb / nab);
  m2 += m2b + delta * delta * (n * (nb / nab));
  n = nab;
}

constexpr int MG_CL = 16;     // channels of a block, adjacent threads
constexpr int MG_L = BLK / MG_CL;  // tile lanes
constexpr int MG_CHAIN = 16;  // partials a lane merges, at most
constexpr int MG_GROUP = MG_L * MG_CHAIN;  // partials a block merges

// in[P][C][2] holds (mean, M2) of the rows [p*span, min(rows, (p+1)*span))
// of every channel; P = ceil(rows / span).  grid = (ceil(C / MG_CL), groups),
// groups = ceil(P / MG_GROUP).  Block (t, g) merges the partials
// [g*MG_GROUP, min(P, (g+1)*MG_GROUP)) of its 16 channels: thread (lane l,
// channel c) the partials g*MG_GROUP + l, + MG_L, ... in ascending order,
// then thread (0, c) the 16 lanes in lane order through LDS.  With one
// group the result is final: save_mean, save_invstd and the running update
// of bn_finalize_kernel.  With more, it is partial g of out[groups][C][2],
// whose span is span*MG_GROUP, and the host launches the kernel again on
// those.  No count is ever stored: every level derives it from (rows, span).
template <bool FINAL>
__global__ __launch_bounds__(BLK) void bn_nhwc_merge_kernel(
    const float* __restrict__ in, uint32_t P, uint32_t span, uint32_t rows,
    uint32_t C, float* __restrict__ out, float eps, float momentum,
    float* __restrict__ save_mean, float* __restrict__ save_invstd,
    float* __restrict__ run_mean, float* __restrict__ run_var) {
  __shared__ float sh[3][MG_L][MG_CL];
  const uint32_t cl = threadIdx.x % MG_CL, l = threadIdx.x / MG_CL;
  const uint32_t c = blockIdx.x * MG_CL + cl;
  const uint32_t p0 = blockIdx.y * MG_GROUP;
  const uint32_t pend = min(P, p0 + MG_GROUP);

  float n = 0.f, mean = 0.f, m2 = 0.f;
  if (c < C) {
    // the loads do not depend on the merges: all in flight together
    float2 v[MG_CHAIN];
#pragma unroll
    for (int j = 0; j < MG_CHAIN; ++j) {
      const uint32_t p = p0 + l + j * MG_L;
      v[j] = *reinterpret_cast<const float2*>(
          in + ((int64_t)(p < pend ? p : p0) * C + c) * 2);
    }
#pragma unroll
    for (int j = 0; j < MG_CHAIN; ++j) {
      const uint32_t p = p0 + l + j * MG_L;
      if (p < pend) {
        const float nb = (float)min(span, rows - p * span);
        if (j == 0) {
          n = nb; mean = v[0].x; m2 = v[0].y;
        } else {
          chan_merge(n, mean, m2, nb, v[j].x, v[j].y);
        }
      }
    }
  }
  sh[0][l][cl] = n;
  sh[1][l][cl] = mean;
  sh[2][l][cl] = m2;
  __syncthreads();
  if (l != 0 || c >= C) return;
  // lane 0 always has a partial; lanes are filled in ascending order
  for (int i = 1; i < MG_L && sh[0][i][cl] > 0.f; ++i)
    chan_merge(n, mean, m2, sh[0][i][cl], sh[1][i][cl], sh[2][i][cl]);
  if (!FINAL) {
    *reinterpret_cast<float2*>(out + ((int64_t)blockIdx.y * C + c) * 2) =
        make_float2(mean, m2);
    return;
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

// ---------------------------------------------------------------------------
// forward apply (+ residual, + ReLU)
// ---------------------------------------------------------------------------
template <typename T, int V>
__global__ __launch_bounds__(BLK) void bn_nhwc_apply_kernel(
    const T* __restrict__ x, const T* __restrict__ res, T* __restrict__ y,
    const float* __restrict__ mean, const float* __restrict__ stat,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    float eps, int eval, int relu, uint32_t rows, uint32_t C, int cl_shift) {
  const ColTile t = col_tile<V>(blockIdx.x, cl_shift, C);
  if (!t.live) return;
  const uint32_t RL = (uint32_t)BLK >> cl_shift;
  float mu[V], sc[V], be[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    float inv;
    channel_stats(mean, stat, eps, eval, t.c + j, mu[j], inv);
    sc[j] = gamma[t.c + j] * inv;
    be[j] = beta[t.c + j];
  }
  for_rows<4>(blockIdx.y * RL + t.rl, rows, gridDim.y * RL, [&](uint32_t r) {
    const uint32_t at = r * C + t.c;
    float f[V], q[V];
    load_vec<T, V>(x + at, f);
    if (res) load_vec<T, V>(res + at, q);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      float v = fmaf(f[j] - mu[j], sc[j], be[j]);
      if (res) v += q[j];
      if (relu) v = v > 0.f ? v : 0.f;
      f[j] = v;
    }
    store_vec<T, V>(y + at, f);
  });
}

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------
template <typename T, int V>
__global__ __launch_bounds__(BLK) void bn_nhwc_bwd_reduce_kernel(
    const T* __restrict__ x, const T* __restrict__ gy,
    const T* __restrict__ y, const float* __restrict__ mean,
    const float* __restrict__ stat, float eps, int eval,
    float* __restrict__ ws, uint32_t rows, uint32_t C, uint32_t per,
    int cl_shift) {
  __shared__ float sh[BLK * V];
  const ColTile t = col_tile<V>(blockIdx.x, cl_shift, C);
  const uint32_t RL = (uint32_t)BLK >> cl_shift;
  const uint32_t r0 = blockIdx.y * per, r1 = min(rows, r0 + per);

  float db[V], dg[V];
#pragma unroll
  for (int j = 0; j < V; ++j) db[j] = dg[j] = 0.f;
  if (t.live) {
    float mu[V], inv[V];
#pragma unroll
    for (int j = 0; j < V; ++j)
      channel_stats(mean, stat, eps, eval, t.c + j, mu[j], inv[j]);
    for_rows<4>(r0 + t.rl, r1, RL, [&](uint32_t r) {
      const uint32_t at = r * C + t.c;
      float fx[V], fg[V], fy[V];
      load_vec<T, V>(x + at, fx);
      load_vec<T, V>(gy + at, fg);
      if (y) load_vec<T, V>(y + at, fy);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float gj = (y && !(fy[j] > 0.f)) ? 0.f : fg[j];
        const float xh = (fx[j] - mu[j]) * inv[j];
        db[j] += gj;
        dg[j] = fmaf(gj, xh, dg[j]);
      }
    });
  }
  const float sdb = lane_combine<V>(db, t, cl_shift, sh);
  const float sdg = lane_combine<V>(dg, t, cl_shift, sh);
  const uint32_t c = (blockIdx.x << cl_shift) * V + threadIdx.x;
  if (threadIdx.x < ((uint32_t)V << cl_shift) && c < C) {
    float* o = ws + ((int64_t)c * gridDim.y + blockIdx.y) * 2;
    o[0] = sdb;
    o[1] = sdg;
  }
}

template <typename T, int V>
__global__ __launch_bounds__(BLK) void bn_nhwc_bwd_apply_kernel(
    const T* __restrict__ x, const T* __restrict__ gy,
    const T* __restrict__ y, const float* __restrict__ mean,
    const float* __restrict__ stat, const float* __restrict__ gamma,
    const float* __restrict__ dgamma, const float* __restrict__ dbeta,
    T* __restrict__ gx, T* __restrict__ gres, float eps, int eval, float n,
    uint32_t rows, uint32_t C, int cl_shift) {
  const ColTile t = col_tile<V>(blockIdx.x, cl_shift, C);
  if (!t.live) return;
  const uint32_t RL = (uint32_t)BLK >> cl_shift;
  float mu[V], inv[V], sc[V], k1[V], k2[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    mu[j] = inv[j] = sc[j] = k1[j] = k2[j] = 0.f;
    if (gx) {
      channel_stats(mean, stat, eps, eval, t.c + j, mu[j], inv[j]);
      sc[j] = gamma[t.c + j] * inv[j];
      if (!eval) {
        k1[j] = dbeta[t.c + j] / n;
        k2[j] = dgamma[t.c + j] / n;
      }
    }
  }
  for_rows<2>(blockIdx.y * RL + t.rl, rows, gridDim.y * RL, [&](uint32_t r) {
    const uint32_t at = r * C + t.c;
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
      float o[V];
      if (eval) {
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = sc[j] * fg[j];
      } else {
        float fx[V];
        load_vec<T, V>(x + at, fx);
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const float xh = (fx[j] - mu[j]) * inv[j];
          o[j] = sc[j] * ((fg[j] - k1[j]) - xh * k2[j]);
        }
      }
      store_vec<T, V>(gx + at, o);
    }
  });
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// The finalize kernels loop over S, so this cap trades their serial merge
// against blocks for the two reduction kernels.  At S = 49..128 a finalize
// launch takes 17..19 us forward and 13..14 us backward where the NCHW
// rule's S <= 32 takes under 5, while 128 slices of one or two column tiles
// still leave the reductions at 128..256 blocks
// (profiles/nhwc_ops_numbers.md has the per-kernel times).
constexpr int MAX_SPLITS = 128;
constexpr int ROWS_PER_LANE = 4;    // at least, in a slice

// How many slices the rows are split into.  Enough blocks to fill the chip
// when channels are few (aim: 8 per CU on 256 CUs, counting column tiles at
// their fp32 width of 4*CL channels), but a slice keeps at least 4 rows per
// row lane, so many channels of few rows are not split to nothing, and at
// most MAX_SPLITS slices, which bounds the serial merge of the finalize
// kernels.  Shapes only: tiles are counted at the fp32 width, so a bf16
// tensor gets half as many blocks (C = 64: one tile of 128 slices).
int batchnorm2d_nhwc_splits(int64_t rows, int64_t C) {
  check_dims(rows, C, 1);
  const int sh = nhwc_cl_shift(C);
  const int64_t ct = (int64_t)4 << sh, rl = BLK >> sh;
  const int64_t tiles = (C + ct - 1) / ct;
  const int64_t want = (2048 + tiles - 1) / tiles;
  const int64_t by_size = rows / (rl * ROWS_PER_LANE);
  int64_t s = std::min(std::min(want, by_size), (int64_t)MAX_SPLITS);
  if (s < 1) s = 1;
  const int64_t per = (rows + s - 1) / s;  // rows per slice
  return (int)((rows + per - 1) / per);    // no empty slice
}

uint32_t rows_per_slice(int64_t rows, int64_t C, int S) {
  if (S != batchnorm2d_nhwc_splits(rows, C))
    throw std::invalid_argument(
        "batchnorm2d_nhwc: splits must come from batchnorm2d_nhwc_splits");
  return (uint32_t)((rows + S - 1) / S);
}

// grid of a kernel that owns V channels per thread: (column tiles, y)
dim3 tile_grid(int64_t C, int v, int sh, int64_t y) {
  const int64_t ct = (int64_t)v << sh;
  return dim3((unsigned)((C + ct - 1) / ct), (unsigned)y);
}

// row blocks of an apply kernel: about 4 rows per thread, at most about
// 4096 blocks in all
int64_t apply_rows_grid(int64_t rows, int64_t C, int v, int sh) {
  const int64_t ct = (int64_t)v << sh, rl = BLK >> sh;
  const int64_t tiles = (C + ct - 1) / ct;
  const int64_t want = (rows + rl * 4 - 1) / (rl * 4);
  return std::min(want, std::max<int64_t>(1, 4096 / tiles));
}

// y from x and the per-channel (mean, stat): the last launch of a forward
void launch_apply(uintptr_t x, uintptr_t res, uintptr_t y, uintptr_t gamma,
                  uintptr_t beta, uintptr_t mean, uintptr_t stat,
                  int64_t rows, int64_t C, bool training, double eps,
                  bool relu, bool is_bf16, uintptr_t stream) {
  const int es = is_bf16 ? 2 : 4, sh = nhwc_cl_shift(C);
  by_dtype_width(is_bf16, pick_v(es, C, {x, res, y}), [&](auto* t, auto v) {
    using T = elem_t<decltype(t)>;
    hipLaunchKernelGGL(
        (bn_nhwc_apply_kernel<T, v()>),
        tile_grid(C, v(), sh, apply_rows_grid(rows, C, v(), sh)), dim3(BLK),
        0, S(stream), (const T*)x, (const T*)res, (T*)y, (const float*)mean,
        (const float*)stat, (const float*)gamma, (const float*)beta,
        (float)eps, (int)!training, (int)relu, (uint32_t)rows, (uint32_t)C,
        sh);
  });
}

// batchnorm2d_fwd's contract on [rows][C] storage, rows = B*H*W
void batchnorm2d_nhwc_fwd(uintptr_t x, uintptr_t res, uintptr_t y,
                          uintptr_t gamma, uintptr_t beta, uintptr_t run_mean,
                          uintptr_t run_var, uintptr_t save_mean,
                          uintptr_t save_invstd, uintptr_t ws, int splits,
                          int64_t rows, int64_t C, bool training,
                          double momentum, double eps, bool relu,
                          bool is_bf16, uintptr_t stream) {
  check_dims(rows, C, 1);
  if (!x || !y || !gamma || !beta)
    throw std::invalid_argument("batchnorm2d_nhwc: null tensor");
  if (!training && (!run_mean || !run_var))
    throw std::invalid_argument(
        "batchnorm2d: eval mode needs the running statistics");
  if (training && (!save_mean || !save_invstd || !ws))
    throw std::invalid_argument(
        "batchnorm2d: training needs save_mean, save_invstd and a workspace");
  if (training && rows < 2)
    throw std::invalid_argument(
        "batchnorm2d: training needs more than one value per channel");
  if ((run_mean == 0) != (run_var == 0))
    throw std::invalid_argument(
        "batchnorm2d: running_mean and running_var come together");
  const int es = is_bf16 ? 2 : 4, sh = nhwc_cl_shift(C);
  if (training) {
    const uint32_t per = rows_per_slice(rows, C, splits);
    by_dtype_width(is_bf16, pick_v(es, C, {x}), [&](auto* t, auto v) {
      using T = elem_t<decltype(t)>;
      hipLaunchKernelGGL((bn_nhwc_stats_kernel<T, v()>),
                         tile_grid(C, v(), sh, splits), dim3(BLK), 0,
                         S(stream), (const T*)x, (float*)ws, (uint32_t)rows,
                         (uint32_t)C, per, sh);
    });
    hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + 63) / 64), dim3(64), 0,
                       S(stream), (const float*)ws, (int)C, splits,
                       (float)eps, (float)momentum, (float*)save_mean,
                       (float*)save_invstd, (float*)run_mean,
                       (float*)run_var);
  }
  launch_apply(x, res, y, gamma, beta, training ? save_mean : run_mean,
               training ? save_invstd : run_var, rows, C, training, eps, relu,
               is_bf16, stream);
  HIP_CHECK(hipGetLastError());
}

// How many floats of workspace batchnorm2d_nhwc_fwd_from_partials needs
// for the levels above the convolution's partials: 0 up to MG_GROUP tiles.
int64_t batchnorm2d_nhwc_merge_ws(int64_t rows, int64_t C) {
  check_dims(rows, C, 1);
  int64_t P = (rows + BN_PARTIAL_ROWS - 1) / BN_PARTIAL_ROWS, n = 0;
  while (P > MG_GROUP) {
    P = (P + MG_GROUP - 1) / MG_GROUP;
    n += P * C * 2;
  }
  return n;
}

// batchnorm2d_nhwc_fwd in training, starting from the partial statistics
// tws[tiles][C][2] = (mean, M2) of x's rows [t*64, min(rows, (t+1)*64)) that
// the convolution which produced x wrote (conv2d_nhwc_bf16_fwd_stats)
// instead of from a pass over x: one merge launch per level (one up to 256
// tiles, two up to 65536, three beyond), then the apply kernel.  ws holds
// batchnorm2d_nhwc_merge_ws(rows, C) floats, 0 where that is 0.
void batchnorm2d_nhwc_fwd_from_partials(
    uintptr_t x, uintptr_t res, uintptr_t y, uintptr_t gamma, uintptr_t beta,
    uintptr_t run_mean, uintptr_t run_var, uintptr_t save_mean,
    uintptr_t save_invstd, uintptr_t tws, uintptr_t ws, int64_t rows,
    int64_t C, double momentum, double eps, bool relu, bool is_bf16,
    uintptr_t stream) {
  check_dims(rows, C, 1);
  if (!x || !y || !gamma || !beta || !save_mean || !save_invstd || !tws)
    throw std::invalid_argument("batchnorm2d_nhwc: null tensor");
  if (tws % 8 || ws % 8)
    throw std::invalid_argument(
        "batchnorm2d_nhwc: the partials must be 8-byte aligned");
  if (rows < 2)
    throw std::invalid_argument(
        "batchnorm2d: training needs more than one value per channel");
  if ((run_mean == 0) != (run_var == 0))
    throw std::invalid_argument(
        "batchnorm2d: running_mean and running_var come together");
  if (!ws && batchnorm2d_nhwc_merge_ws(rows, C) > 0)
    throw std::invalid_argument("batchnorm2d_nhwc: no merge workspace");
  const float* in = (const float*)tws;
  float* next = (float*)ws;
  int64_t span = BN_PARTIAL_ROWS;
  int64_t P = (rows + span - 1) / span;
  const unsigned ctiles = (unsigned)((C + MG_CL - 1) / MG_CL);
  while (P > MG_GROUP) {  // span * MG_GROUP < rows: fits 32 bits
    const int64_t groups = (P + MG_GROUP - 1) / MG_GROUP;
    hipLaunchKernelGGL(bn_nhwc_merge_kernel<false>,
                       dim3(ctiles, (unsigned)groups), dim3(BLK), 0,
                       S(stream), in, (uint32_t)P, (uint32_t)span,
                       (uint32_t)rows, (uint32_t)C, next, 0.f, 0.f,
                       (float*)nullptr, (float*)nullptr, (float*)nullptr,
                       (float*)nullptr);
    in = next;
    next += groups * C * 2;
    span *= MG_GROUP;
    P = groups;
  }
  hipLaunchKernelGGL(bn_nhwc_merge_kernel<true>, dim3(ctiles, 1), dim3(BLK),
                     0, S(stream), in, (uint32_t)P, (uint32_t)span,
                     (uint32_t)rows, (uint32_t)C, (float*)nullptr, (float)eps,
                     (float)momentum, (float*)save_mean, (float*)save_invstd,
                     (float*)run_mean, (float*)run_var);
  launch_apply(x, res, y, gamma, beta, save_mean, save_invstd, rows, C, true,
               eps, relu, is_bf16, stream);
  HIP_CHECK(hipGetLastError());
}

// batchnorm2d_bwd's contract on [rows][C] storage
void batchnorm2d_nhwc_bwd(uintptr_t x, uintptr_t gy, uintptr_t y,
                          uintptr_t gamma, uintptr_t mean, uintptr_t stat,
                          uintptr_t dgamma, uintptr_t dbeta, uintptr_t gx,
                          uintptr_t gres, uintptr_t ws, int splits,
                          int64_t rows, int64_t C, bool training, double eps,
                          bool is_bf16, uintptr_t stream) {
  check_dims(rows, C, 1);
  if (!x || !gy || !mean || !stat || !gamma || !dgamma || !dbeta || !ws)
    throw std::invalid_argument("batchnorm2d_nhwc_bwd: null tensor");
  const int es = is_bf16 ? 2 : 4, sh = nhwc_cl_shift(C);
  const uint32_t per = rows_per_slice(rows, C, splits);
  const int eval = !training;
  by_dtype_width(is_bf16, pick_v(es, C, {x, gy, y}), [&](auto* t, auto v) {
    using T = elem_t<decltype(t)>;
    hipLaunchKernelGGL((bn_nhwc_bwd_reduce_kernel<T, v()>),
                       tile_grid(C, v(), sh, splits), dim3(BLK), 0, S(stream),
                       (const T*)x, (const T*)gy, (const T*)y,
                       (const float*)mean, (const float*)stat, (float)eps,
                       eval, (float*)ws, (uint32_t)rows, (uint32_t)C, per, sh);
  });
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((C + 63) / 64), dim3(64), 0,
                     S(stream), (const float*)ws, (int)C, splits,
                     (float*)dgamma, (float*)dbeta);
  if (gx || gres)
    by_dtype_width(
        is_bf16, pick_v(es, C, {x, gy, y, gx, gres}), [&](auto* t, auto v) {
          using T = elem_t<decltype(t)>;
          hipLaunchKernelGGL(
              (bn_nhwc_bwd_apply_kernel<T, v()>),
              tile_grid(C, v(), sh, apply_rows_grid(rows, C, v(), sh)),
              dim3(BLK), 0, S(stream), (const T*)x, (const T*)gy,
              (const T*)y, (const float*)mean, (const float*)stat,
              (const float*)gamma, (const float*)dgamma, (const float*)dbeta,
              (T*)gx, (T*)gres, (float)eps, eval, (float)rows, (uint32_t)rows,
              (uint32_t)C, sh);
        });
  HIP_CHECK(hipGetLastError());
}

}  // namespace

void register_batchnorm_nhwc(pybind11::module_& m) {
  m.def("batchnorm2d_nhwc_splits", &batchnorm2d_nhwc_splits);
  m.def("batchnorm2d_nhwc_fwd", &batchnorm2d_nhwc_fwd);
  m.def("batchnorm2d_nhwc_merge_ws", &batchnorm2d_nhwc_merge_ws);
  m.def("batchnorm2d_nhwc_fwd_from_partials",
        &batchnorm2d_nhwc_fwd_from_partials);
  m.def("batchnorm2d_nhwc_bwd", &batchnorm2d_nhwc_bwd);
}
