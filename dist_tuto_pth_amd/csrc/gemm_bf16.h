// gemm_bf16.h — the bf16 MFMA tile GEMM that linear_bf16.hip (K16) and
// conv_bf16.hip (K17) share.
//
// One block computes a 64x64 tile of
//     C[m][n] = sum_k A(m,k) * B(n,k)
// on v_mfma_f32_16x16x32_bf16 with fp32 accumulators, from two LDS tiles
// As[m][k], Bs[n][k].  Both are K-contiguous, so an MFMA fragment is one
// 16-byte LDS read.  What differs per product is
//   - the loaders: global -> registers (one K tile ahead) -> LDS.  A
//     loader fills this thread's NPASS chunks of a 64x64 operand tile;
//     out-of-range and padded elements arrive as zero.
//   - the epilogue: a functor that stores element (split z, m, n).
//
// Everything here has internal linkage: each translation unit that
// includes the header gets its own copy.

#pragma once

#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 frag_ab;
typedef __attribute__((ext_vector_type(4))) float frag_cd;

static_assert(BLK == 256, "the block is 2x2 waves");
constexpr int BM = 64;         // block tile rows
constexpr int BN = 64;         // block tile cols
constexpr int BK = 64;         // reduction depth per LDS tile
constexpr int LDS_LD = BK + 8; // 144-byte rows: 16-byte aligned; the
                               // 36-dword pitch puts 8 consecutive rows in
                               // 8 different 4-bank groups for the 16-byte
                               // fragment reads
constexpr int NPASS = BM * BK / (BLK * 8);  // 8-element chunks per thread
static_assert(BK == 64, "lds_col swizzles the 8 chunks of a 64-deep row");

// Column swizzle of the LDS tiles.  A transposed write sends the 8 lanes
// that share a k to rows 8 apart; 8 rows are 288 dwords = 32 banks, so
// unswizzled they would alternate between two banks.  XOR-ing the 8-element
// chunk index with the row's 8-row group moves them to 8 different chunks.
// Chunks stay whole, so fragment reads remain one aligned 16-byte read.
__device__ __forceinline__ int lds_col(int row, int col) {
  return col ^ (((row >> 3) & 7) << 3);
}

using Chunk = Vec<bf16_t, 8>;  // 8 bf16 as one 16-byte value (common.h)

__device__ __forceinline__ Chunk zero_chunk() {
  Chunk c;
  c.raw = make_uint4(0u, 0u, 0u, 0u);
  return c;
}

// Which chunk of a 64x64 operand tile thread `tid` owns in pass `p`: `hi`
// (0..63) counts whole rows of chunks, `lo` (0,8,..,56) is the chunk's
// first element along the other axis.  A plain loader puts rows on `hi`
// and k on `lo` (chunk runs along k); a transposed one puts k on `hi` and
// rows on `lo` (chunk runs along the rows).
__device__ __forceinline__ int chunk_hi(int p, int tid) {
  return p * (BLK / 8) + (tid >> 3);
}
__device__ __forceinline__ int chunk_lo(int tid) { return (tid & 7) * 8; }

template <bool TRANS>
__device__ __forceinline__ void lds_store(bf16_t (*T)[LDS_LD], int tid,
                                          const Chunk (&reg)[NPASS]) {
#pragma unroll
  for (int p = 0; p < NPASS; ++p) {
    const int hi = chunk_hi(p, tid);
    const int lo = chunk_lo(tid);
    if (!TRANS) {
      *reinterpret_cast<uint4*>(&T[hi][lds_col(hi, lo)]) = reg[p].raw;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        T[lo + j][lds_col(lo + j, hi)] = reg[p].e[j];
    }
  }
}

// ---------------------------------------------------------------------------
// plain (dense, row-major) operand loader
// ---------------------------------------------------------------------------
struct Operand {
  const bf16_t* p;   // element (r, k): p[r*ld + k], or p[k*ld + r] if TRANS
  int64_t ld;
  int rows;          // valid r in [0, rows)
  int vec;           // 16-byte global loads are aligned for this operand
  const void* mask;  // same indexing as p; element kept where mask > 0
  int mask_f32;      // mask dtype: fp32 (1) or bf16 (0)
};

__device__ __forceinline__ Chunk load8(const Operand& o, int64_t idx,
                                       int nvalid) {
  // nvalid = how many of the 8 consecutive elements from idx are in range
  Chunk c;
  c.raw = make_uint4(0u, 0u, 0u, 0u);
  if (nvalid <= 0) return c;
  if (o.vec && nvalid >= 8) {
    c.raw = *reinterpret_cast<const uint4*>(o.p + idx);
    if (o.mask) {
      if (o.mask_f32) {
        const float4* m =
            reinterpret_cast<const float4*>((const float*)o.mask + idx);
        const float4 m0 = m[0], m1 = m[1];
        if (!(m0.x > 0.f)) c.e[0] = 0; if (!(m0.y > 0.f)) c.e[1] = 0;
        if (!(m0.z > 0.f)) c.e[2] = 0; if (!(m0.w > 0.f)) c.e[3] = 0;
        if (!(m1.x > 0.f)) c.e[4] = 0; if (!(m1.y > 0.f)) c.e[5] = 0;
        if (!(m1.z > 0.f)) c.e[6] = 0; if (!(m1.w > 0.f)) c.e[7] = 0;
      } else {
        Chunk m;
        m.raw = *reinterpret_cast<const uint4*>((const bf16_t*)o.mask + idx);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (!(to_f(m.e[j]) > 0.f)) c.e[j] = 0;
      }
    }
    return c;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (j < nvalid) {
      bf16_t v = o.p[idx + j];
      if (o.mask) {
        const float m = o.mask_f32 ? ((const float*)o.mask)[idx + j]
                                   : to_f(((const bf16_t*)o.mask)[idx + j]);
        if (!(m > 0.f)) v = 0;
      }
      c.e[j] = v;
    }
  }
  return c;
}

// Fetch this thread's chunks of the tile rows [r0, r0+64) x k [k0, k0+64),
// k clipped to kend.  Out-of-range elements come back as zero.
template <bool TRANS>
__device__ __forceinline__ void gload(const Operand& o, int r0, int k0,
                                      int kend, int tid, Chunk (&reg)[NPASS]) {
#pragma unroll
  for (int p = 0; p < NPASS; ++p) {
    const int hi = p * (BLK / 8) + (tid >> 3);  // 0..63
    const int lo = (tid & 7) * 8;              // 0,8,..,56
    if (!TRANS) {
      const int r = r0 + hi, k = k0 + lo;      // chunk runs along k
      const int nvalid = (r < o.rows) ? (kend - k) : 0;
      reg[p] = load8(o, (int64_t)r * o.ld + k, nvalid);
    } else {
      const int k = k0 + hi, r = r0 + lo;      // chunk runs along r
      const int nvalid = (k < kend) ? (o.rows - r) : 0;
      reg[p] = load8(o, (int64_t)k * o.ld + r, nvalid);
    }
  }
}

template <bool TRANS>
struct PlainLoader {
  Operand o;
  __device__ __forceinline__ void load(int r0, int k0, int kend, int tid,
                                       Chunk (&reg)[NPASS]) const {
    gload<TRANS>(o, r0, k0, kend, tid, reg);
  }
};

// Pitch of the fp32 C tile a tiled epilogue stages in LDS as Ct[n][m]:
// rows stay 16-byte aligned, so an accumulator fragment (4 consecutive m)
// is one 16-byte write.
constexpr int CT_LD = BM + 4;

// Epilogues.  An element-wise one (kTiled == false) is handed each
// (z, m, n, value) from the accumulator registers.  A tiled one
// (kTiled == true) is for outputs that are contiguous along m, not n: the
// block stages its C tile in LDS and store_tile() writes it out along m.

// row-major epilogue: C[z][m][n]
template <typename OutT>
struct RowMajorOut {
  static constexpr bool kTiled = false;
  OutT* C;
  int M, N;
  __device__ __forceinline__ void operator()(int z, int m, int n,
                                             float v) const {
    from_f(v, C[((int64_t)z * M + m) * N + n]);
  }
};

// ---------------------------------------------------------------------------
// the GEMM:  C[m][n] = sum_{k in split} A(m,k) * B(n,k)   (+bias[n]) (ReLU)
// grid = (m tiles, n tiles, splits); split z reduces k in
// [z*kchunk, min(Kred, (z+1)*kchunk)) and hands the result to `epi`.
// colsum (gw only): colsum[z*M + m] = sum_k A(m,k), written by the n-tile-0
// blocks — that is gb (or its split partial).
//
// LA / LB:  void load(int r0, int k0, int kend, int tid,
//                     Chunk (&reg)[NPASS]) const
// fetches the tile rows [r0, r0+64) x k [k0, k0+64), k clipped to kend, in
// the chunk layout of TA / TB (see chunk_hi).
// ---------------------------------------------------------------------------
template <bool TA, bool TB, class LA, class LB, class Epi>
__device__ __forceinline__ void gemm_bf16_block(
    const LA& A, const LB& B, int M, int N, int Kred, int kchunk,
    const float* __restrict__ bias, int relu, float* __restrict__ colsum,
    const Epi& epi) {
  __shared__ __attribute__((aligned(16))) bf16_t As[BM][LDS_LD];
  __shared__ __attribute__((aligned(16))) bf16_t Bs[BN][LDS_LD];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const int kbeg = blockIdx.z * kchunk;
  const int kend = min(Kred, kbeg + kchunk);
  const bool do_colsum = colsum != nullptr && blockIdx.y == 0;

  frag_cd acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = frag_cd{0.f, 0.f, 0.f, 0.f};
  float csum = 0.f;

  Chunk ra[NPASS], rb[NPASS];
  if (kbeg < kend) {
    A.load(m0, kbeg, kend, tid, ra);
    B.load(n0, kbeg, kend, tid, rb);
  }
  for (int k0 = kbeg; k0 < kend; k0 += BK) {
    lds_store<TA>(As, tid, ra);
    lds_store<TB>(Bs, tid, rb);
    __syncthreads();
    if (k0 + BK < kend) {  // next tile's global loads fly under the MFMAs
      A.load(m0, k0 + BK, kend, tid, ra);
      B.load(n0, k0 + BK, kend, tid, rb);
    }
#pragma unroll
    for (int ks = 0; ks < BK; ks += 32) {
      const int kk = ks + 8 * (lane >> 4);
      frag_ab a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int ar = wm + i * 16 + (lane & 15);
        const int br = wn + i * 16 + (lane & 15);
        a[i] = *reinterpret_cast<const frag_ab*>(&As[ar][lds_col(ar, kk)]);
        b[i] = *reinterpret_cast<const frag_ab*>(&Bs[br][lds_col(br, kk)]);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a[i], b[j], acc[i][j], 0, 0, 0);
    }
    if (do_colsum) {  // 4 threads per row, 2 chunks each, fixed order
      const bf16_t* row = &As[tid >> 2][(tid & 3) * 16];
#pragma unroll
      for (int j = 0; j < 16; ++j) csum += to_f(row[j]);
    }
    __syncthreads();
  }

  if constexpr (Epi::kTiled) {
    __shared__ __attribute__((aligned(16))) float Ct[BN][CT_LD];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int nl = wn + j * 16 + (lane & 15);
        const int ml = wm + i * 16 + (lane >> 4) * 4;
        const float bv = (bias && n0 + nl < N) ? bias[n0 + nl] : 0.f;
        float4 v = make_float4(acc[i][j][0] + bv, acc[i][j][1] + bv,
                               acc[i][j][2] + bv, acc[i][j][3] + bv);
        if (relu) {
          v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f);
          v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
        }
        *reinterpret_cast<float4*>(&Ct[nl][ml]) = v;
      }
    __syncthreads();
    epi.store_tile(Ct, m0, n0, M, tid);
  } else {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int n = n0 + wn + j * 16 + (lane & 15);
        if (n >= N) continue;
        const float bv = bias ? bias[n] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = m0 + wm + i * 16 + (lane >> 4) * 4 + r;
          if (m >= M) continue;
          float v = acc[i][j][r] + bv;
          if (relu) v = fmaxf(v, 0.f);
          epi((int)blockIdx.z, m, n, v);
        }
      }
  }

  if (do_colsum) {
    csum += __shfl_xor(csum, 1);
    csum += __shfl_xor(csum, 2);
    const int m = m0 + (tid >> 2);
    if ((tid & 3) == 0 && m < M) colsum[(int64_t)blockIdx.z * M + m] = csum;
  }
}

// gw[i] = sum_s part[s][i]; gb[n] = sum_s gb_part[s][n] — split order, so
// the result does not depend on scheduling.
__global__ void gw_combine_kernel(const float* __restrict__ part,
                                  float* __restrict__ gw, int64_t n_gw,
                                  const float* __restrict__ gb_part,
                                  float* __restrict__ gb, int n_gb,
                                  int splits) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nth = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = tid; i < n_gw; i += nth) {
    float s = 0.f;
    for (int z = 0; z < splits; ++z) s += part[(int64_t)z * n_gw + i];
    gw[i] = s;
  }
  if (gb)
    for (int64_t i = tid; i < n_gb; i += nth) {
      float s = 0.f;
      for (int z = 0; z < splits; ++z) s += gb_part[(int64_t)z * n_gb + i];
      gb[i] = s;
    }
}

inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// Division of 0 <= n < 2^31 by a divisor fixed at launch, as one multiply-
// high and a shift (Granlund & Montgomery): the loaders and the NCHW
// epilogue take indices apart many times per tile.
struct FastDiv {
  uint32_t d, mul, shr;
  __device__ __forceinline__ int div(int n) const {
    return d == 1 ? n : (int)(__umulhi((uint32_t)n, mul) >> shr);
  }
};

inline FastDiv fast_div(int d) {
  FastDiv f{(uint32_t)d, 0u, 0u};
  if (d <= 1) return f;
  uint32_t l = 0;
  while ((1ull << l) < (uint64_t)d) ++l;  // 2^l >= d
  const uint32_t p = 31 + l;
  f.mul = (uint32_t)(((1ull << p) + (uint64_t)d - 1) / (uint64_t)d);
  f.shr = p - 32;
  return f;
}

inline Operand operand(uintptr_t p, int64_t ld, int rows, uintptr_t mask = 0,
                       bool mask_f32 = false) {
  Operand o;
  o.p = (const bf16_t*)p;
  o.ld = ld;
  o.rows = rows;
  o.vec = (ld % 8 == 0) && (p % 16 == 0) && (mask % 16 == 0);
  o.mask = (const void*)mask;
  o.mask_f32 = mask_f32;
  return o;
}

// How many reduction splits a weight-gradient GEMM of M x N over `red`
// uses: enough blocks to cover the 256 CUs twice, each split at least two
// LDS tiles deep, no empty trailing split.
inline int gw_split_count(int red, int M, int N) {
  const int64_t tiles = (int64_t)cdiv(M, BM) * cdiv(N, BN);
  const int64_t want = (512 + tiles - 1) / tiles;
  const int64_t most = cdiv(red, 2 * BK);
  int64_t s = want < most ? want : most;
  if (s < 1) s = 1;
  const int kchunk = cdiv(cdiv(red, (int)s), BK) * BK;
  return cdiv(red, kchunk);
}

inline int gw_split_chunk(int red, int splits) {
  return cdiv(cdiv(red, splits), BK) * BK;
}

}  // namespace
