// K16 — bf16 mixed-precision linear on the CDNA4 matrix cores (gfx950).
//
// Numeric contract (ops.linear_bf16): every GEMM operand is bf16, products
// accumulate in fp32 on v_mfma_f32_16x16x32_bf16, and each result is rounded
// ONCE (RNE) from the fp32 accumulator to its output dtype.  fp32 operands
// (master weights, the first layer's input, an fp32 upstream gradient) are
// rounded to bf16 by cast_f32_to_bf16 first.
//
// One GEMM kernel serves all three products.  It computes
//     C[m][n] = sum_k A(m,k) * B(n,k)
// from two LDS tiles As[m][k], Bs[n][k] (both K-contiguous, so MFMA
// fragments are one 16-byte LDS read each); what differs per product is the
// global->LDS loader:
//     forward   out = x  · wᵀ   A = x  plain        B = w plain
//     gx            = gy'· w    A = gy plain+mask   B = w transposed on write
//     gw            = gy'ᵀ· x   A = gy transposed+mask, B = x transposed
// gy' = gy where the saved (ReLU-fused) output is > 0; the mask is applied
// while gy is staged.  gw is fp32 and split over the batch through a
// partial buffer that a second kernel sums in split order: no float
// atomics, bitwise reproducible.  gb rides along in the gw kernel.
//
// Bindings are registered from kernels.hip's PYBIND11_MODULE through
// register_linear_bf16().

#include "common.h"

#include <pybind11/pybind11.h>

namespace {

using bf16_t = uint16_t;  // raw bits; all arithmetic goes through fp32
typedef __attribute__((ext_vector_type(8))) __bf16 frag_ab;
typedef __attribute__((ext_vector_type(4))) float frag_cd;

constexpr int NT = 256;        // threads per block (4 waves, 2x2)
constexpr int BM = 64;         // block tile rows
constexpr int BN = 64;         // block tile cols
constexpr int BK = 64;         // reduction depth per LDS tile
constexpr int LDS_LD = BK + 8; // 144-byte rows: 16-byte aligned; the
                               // 36-dword pitch puts 8 consecutive rows in
                               // 8 different 4-bank groups for the 16-byte
                               // fragment reads
constexpr int NPASS = BM * BK / (NT * 8);  // 8-element chunks per thread
static_assert(BK == 64, "lds_col swizzles the 8 chunks of a 64-deep row");

// Column swizzle of the LDS tiles.  A transposed write sends the 8 lanes
// that share a k to rows 8 apart; 8 rows are 288 dwords = 32 banks, so
// unswizzled they would alternate between two banks.  XOR-ing the 8-element
// chunk index with the row's 8-row group moves them to 8 different chunks.
// Chunks stay whole, so fragment reads remain one aligned 16-byte read.
__device__ __forceinline__ int lds_col(int row, int col) {
  return col ^ (((row >> 3) & 7) << 3);
}

__device__ __forceinline__ float bf2f(bf16_t v) {
  return __uint_as_float((uint32_t)v << 16);
}

// fp32 -> bf16, round-to-nearest-even, NaN kept quiet (torch's rule)
__device__ __forceinline__ bf16_t f2bf(float f) {
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (bf16_t)0x7fc0;
  u += 0x7fffu + ((u >> 16) & 1u);
  return (bf16_t)(u >> 16);
}

__device__ __forceinline__ void store_out(float* p, float v) { *p = v; }
__device__ __forceinline__ void store_out(bf16_t* p, float v) { *p = f2bf(v); }

union Chunk {  // 8 bf16
  uint4 v;
  bf16_t e[8];
};

// ---------------------------------------------------------------------------
// cast fp32 -> bf16
// ---------------------------------------------------------------------------
__global__ void cast_f32_to_bf16_kernel(const float* __restrict__ src,
                                        bf16_t* __restrict__ dst, int64_t n,
                                        int64_t nvec) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nth = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = tid; i < nvec; i += nth) {
    const float4 a = reinterpret_cast<const float4*>(src)[2 * i];
    const float4 b = reinterpret_cast<const float4*>(src)[2 * i + 1];
    Chunk c;
    c.e[0] = f2bf(a.x); c.e[1] = f2bf(a.y);
    c.e[2] = f2bf(a.z); c.e[3] = f2bf(a.w);
    c.e[4] = f2bf(b.x); c.e[5] = f2bf(b.y);
    c.e[6] = f2bf(b.z); c.e[7] = f2bf(b.w);
    reinterpret_cast<uint4*>(dst)[i] = c.v;
  }
  for (int64_t i = nvec * 8 + tid; i < n; i += nth) dst[i] = f2bf(src[i]);
}

// ---------------------------------------------------------------------------
// loaders: global -> registers (one K tile ahead) -> LDS
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
  c.v = make_uint4(0u, 0u, 0u, 0u);
  if (nvalid <= 0) return c;
  if (o.vec && nvalid >= 8) {
    c.v = *reinterpret_cast<const uint4*>(o.p + idx);
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
        m.v = *reinterpret_cast<const uint4*>((const bf16_t*)o.mask + idx);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (!(bf2f(m.e[j]) > 0.f)) c.e[j] = 0;
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
                                   : bf2f(((const bf16_t*)o.mask)[idx + j]);
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
    const int hi = p * (NT / 8) + (tid >> 3);  // 0..63
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
__device__ __forceinline__ void lds_store(bf16_t (*T)[LDS_LD], int tid,
                                          const Chunk (&reg)[NPASS]) {
#pragma unroll
  for (int p = 0; p < NPASS; ++p) {
    const int hi = p * (NT / 8) + (tid >> 3);
    const int lo = (tid & 7) * 8;
    if (!TRANS) {
      *reinterpret_cast<uint4*>(&T[hi][lds_col(hi, lo)]) = reg[p].v;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        T[lo + j][lds_col(lo + j, hi)] = reg[p].e[j];
    }
  }
}

// ---------------------------------------------------------------------------
// the GEMM:  C[m][n] = sum_{k in split} A(m,k) * B(n,k)   (+bias[n]) (ReLU)
// grid = (m tiles, n tiles, splits); split z reduces k in
// [z*kchunk, min(Kred, (z+1)*kchunk)) and writes C + z*M*N.
// colsum (gw only): colsum[z*M + m] = sum_k A(m,k), written by the n-tile-0
// blocks — that is gb (or its split partial).
// ---------------------------------------------------------------------------
template <bool TA, bool TB, typename OutT>
__global__ __launch_bounds__(NT) void gemm_bf16_kernel(
    Operand A, Operand B, int Kred, int kchunk, OutT* __restrict__ C,
    const float* __restrict__ bias, int relu, float* __restrict__ colsum) {
  __shared__ __attribute__((aligned(16))) bf16_t As[BM][LDS_LD];
  __shared__ __attribute__((aligned(16))) bf16_t Bs[BN][LDS_LD];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const int M = A.rows, N = B.rows;
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
    gload<TA>(A, m0, kbeg, kend, tid, ra);
    gload<TB>(B, n0, kbeg, kend, tid, rb);
  }
  for (int k0 = kbeg; k0 < kend; k0 += BK) {
    lds_store<TA>(As, tid, ra);
    lds_store<TB>(Bs, tid, rb);
    __syncthreads();
    if (k0 + BK < kend) {  // next tile's global loads fly under the MFMAs
      gload<TA>(A, m0, k0 + BK, kend, tid, ra);
      gload<TB>(B, n0, k0 + BK, kend, tid, rb);
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
      for (int j = 0; j < 16; ++j) csum += bf2f(row[j]);
    }
    __syncthreads();
  }

  OutT* Cz = C + (int64_t)blockIdx.z * M * N;
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
        store_out(Cz + (int64_t)m * N + n, v);
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

// ---------------------------------------------------------------------------
// bf16 elementwise dropout: the RNG (mix32) and the seed advance
// (launch_bump_seed) ARE the fp32 kernels' (common.h), and the element index
// and seed pointer are the same, so equal (seed, p) gives equal masks.
// ---------------------------------------------------------------------------
__global__ void dropout_bf16_fwd_kernel(
    const bf16_t* __restrict__ x, bf16_t* __restrict__ out,
    uint8_t* __restrict__ mask, int64_t n, float p, float scale,
    const unsigned long long* __restrict__ sp) {
  const uint32_t thresh = (uint32_t)(p * 4294967296.0);
  const uint64_t seed = sp[0];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t r = mix32(seed, (uint64_t)i) << 16 |
                 (mix32(seed ^ 0xabcd, i) & 0xffff);
    uint8_t keep = r >= thresh;
    mask[i] = keep;
    out[i] = keep ? f2bf(bf2f(x[i]) * scale) : (bf16_t)0;
  }
}

__global__ void dropout_bf16_bwd_kernel(const bf16_t* __restrict__ gy,
                                        const uint8_t* __restrict__ mask,
                                        bf16_t* __restrict__ gx, int64_t n,
                                        float scale) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    gx[i] = mask[i] ? f2bf(bf2f(gy[i]) * scale) : (bf16_t)0;
}

// ---------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------
static inline int ew_grid(int64_t work) {
  int64_t g = (work + NT - 1) / NT;
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  return (int)g;
}

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }

static Operand operand(uintptr_t p, int64_t ld, int rows, uintptr_t mask = 0,
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

static void check_dims(int B, int K, int N) {
  if (B < 1 || K < 1 || N < 1)
    throw std::invalid_argument("linear_bf16: B, K, N must be >= 1");
}

void cast_f32_to_bf16(uintptr_t src, uintptr_t dst, int64_t n,
                      uintptr_t stream) {
  if (n <= 0) return;
  const int64_t nvec = (src % 16 == 0 && dst % 16 == 0) ? n / 8 : 0;
  hipLaunchKernelGGL(cast_f32_to_bf16_kernel, dim3(ew_grid((n + 7) / 8)),
                     dim3(NT), 0, S(stream), (const float*)src, (bf16_t*)dst,
                     n, nvec);
}

// out[B,N] = x[B,K] · w[N,K]ᵀ (+ bias) (ReLU); x, w bf16
void linear_bf16_fwd(uintptr_t x, uintptr_t w, uintptr_t bias, uintptr_t out,
                     int B, int K, int N, bool relu, bool out_f32,
                     uintptr_t stream) {
  check_dims(B, K, N);
  const Operand a = operand(x, K, B), b = operand(w, K, N);
  const dim3 grid(cdiv(B, BM), cdiv(N, BN), 1);
  if (out_f32)
    hipLaunchKernelGGL((gemm_bf16_kernel<false, false, float>), grid,
                       dim3(NT), 0, S(stream), a, b, K, K, (float*)out,
                       (const float*)bias, (int)relu, (float*)nullptr);
  else
    hipLaunchKernelGGL((gemm_bf16_kernel<false, false, bf16_t>), grid,
                       dim3(NT), 0, S(stream), a, b, K, K, (bf16_t*)out,
                       (const float*)bias, (int)relu, (float*)nullptr);
}

// gx[B,K] = gy'[B,N] · w[N,K]; mask (the saved output, 0 = none) has gy's
// layout and is bf16 or fp32
void linear_bf16_bwd_x(uintptr_t gy, uintptr_t w, uintptr_t mask,
                       bool mask_f32, uintptr_t gx, int B, int K, int N,
                       bool out_f32, uintptr_t stream) {
  check_dims(B, K, N);
  const Operand a = operand(gy, N, B, mask, mask_f32);
  const Operand b = operand(w, K, K);  // B(n=k_col, k=n) = w[n*K + k_col]
  const dim3 grid(cdiv(B, BM), cdiv(K, BN), 1);
  if (out_f32)
    hipLaunchKernelGGL((gemm_bf16_kernel<false, true, float>), grid, dim3(NT),
                       0, S(stream), a, b, N, N, (float*)gx,
                       (const float*)nullptr, 0, (float*)nullptr);
  else
    hipLaunchKernelGGL((gemm_bf16_kernel<false, true, bf16_t>), grid,
                       dim3(NT), 0, S(stream), a, b, N, N, (bf16_t*)gx,
                       (const float*)nullptr, 0, (float*)nullptr);
}

// How many batch splits the weight gradient uses: enough blocks to cover
// the 256 CUs twice, each split at least two LDS tiles deep.
int linear_bf16_gw_splits(int B, int K, int N) {
  check_dims(B, K, N);
  const int64_t tiles = (int64_t)cdiv(N, BM) * cdiv(K, BN);
  const int64_t want = (512 + tiles - 1) / tiles;
  const int64_t most = cdiv(B, 2 * BK);
  int64_t s = want < most ? want : most;
  if (s < 1) s = 1;
  const int kchunk = cdiv(cdiv(B, (int)s), BK) * BK;
  return cdiv(B, kchunk);  // no empty trailing split
}

// gw[N,K] = gy'ᵀ · x (fp32), gb[N] = sum_b gy' (fp32, 0 = skip).
// part: fp32 workspace of splits*(N*K + N) floats (unused when splits == 1).
void linear_bf16_bwd_w(uintptr_t gy, uintptr_t x, uintptr_t mask,
                       bool mask_f32, uintptr_t gw, uintptr_t gb,
                       uintptr_t part, int splits, int B, int K, int N,
                       uintptr_t stream) {
  check_dims(B, K, N);
  if (splits != linear_bf16_gw_splits(B, K, N))
    throw std::invalid_argument("linear_bf16_bwd_w: wrong split count");
  const Operand a = operand(gy, N, N, mask, mask_f32);  // A(n, b)
  const Operand b = operand(x, K, K);                   // B(k, b)
  const int kchunk = cdiv(cdiv(B, splits), BK) * BK;
  const dim3 grid(cdiv(N, BM), cdiv(K, BN), splits);
  const int64_t n_gw = (int64_t)N * K;
  float* c = (float*)gw;
  float* cs = (float*)gb;
  if (splits > 1) {
    if (!part) throw std::invalid_argument("linear_bf16_bwd_w: no workspace");
    c = (float*)part;
    cs = gb ? c + (int64_t)splits * n_gw : nullptr;
  }
  hipLaunchKernelGGL((gemm_bf16_kernel<true, true, float>), grid, dim3(NT), 0,
                     S(stream), a, b, B, kchunk, c, (const float*)nullptr, 0,
                     cs);
  if (splits > 1)
    hipLaunchKernelGGL(gw_combine_kernel, dim3(ew_grid(n_gw)), dim3(NT), 0,
                       S(stream), (const float*)c, (float*)gw, n_gw,
                       (const float*)cs, (float*)gb, N, splits);
}

void dropout_bf16_fwd(uintptr_t x, uintptr_t out, uintptr_t mask, int64_t n,
                      double p, uintptr_t seed_dev, uintptr_t stream) {
  const float scale = 1.f / (1.f - (float)p);
  launch_bump_seed(seed_dev, S(stream));
  hipLaunchKernelGGL(dropout_bf16_fwd_kernel, dim3(ew_grid(n)), dim3(NT), 0,
                     S(stream), (const bf16_t*)x, (bf16_t*)out,
                     (uint8_t*)mask, n, (float)p, scale,
                     (const unsigned long long*)seed_dev);
}

void dropout_bf16_bwd(uintptr_t gy, uintptr_t mask, uintptr_t gx, int64_t n,
                      double scale, uintptr_t stream) {
  hipLaunchKernelGGL(dropout_bf16_bwd_kernel, dim3(ew_grid(n)), dim3(NT), 0,
                     S(stream), (const bf16_t*)gy, (const uint8_t*)mask,
                     (bf16_t*)gx, n, (float)scale);
}

}  // namespace

void register_linear_bf16(pybind11::module_& m) {
  m.def("cast_f32_to_bf16", &cast_f32_to_bf16);
  m.def("linear_bf16_fwd", &linear_bf16_fwd);
  m.def("linear_bf16_bwd_x", &linear_bf16_bwd_x);
  m.def("linear_bf16_gw_splits", &linear_bf16_gw_splits);
  m.def("linear_bf16_bwd_w", &linear_bf16_bwd_w);
  m.def("dropout_bf16_fwd", &dropout_bf16_fwd);
  m.def("dropout_bf16_bwd", &dropout_bf16_bwd);
}
