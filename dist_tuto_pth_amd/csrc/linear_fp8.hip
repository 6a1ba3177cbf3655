// K22 — fp8 linear on the CDNA4 128-deep matrix instruction (gfx950).
//
// Numeric contract (ops.linear_fp8): per-tensor, current, power-of-two
// scaling.  x and w are quantised to e4m3, the incoming gradient to e5m2;
// a tensor with amax = f * 2^e, f in [1,2), gets s = 2^k with k = E - e for
// f <= 1.75 and E - 1 - e otherwise (E = 8 for e4m3, 15 for e5m2), k clamped
// to [-126, 126], k = 0 for amax == 0.  The quantised value is RNE_fp8(t*s),
// by v_cvt_pk_fp8_f32 / v_cvt_pk_bf8_f32.  Products are exact in fp32 and
// are summed by v_mfma_scale_f32_16x16x128_f8f6f4 (block scales fixed at 1)
// into an fp32 accumulator; the accumulator is multiplied by the two exact
// 1/s, bias is added, ReLU applied, and the result rounded ONCE to its
// output dtype.  s and 1/s never leave the device.
// The instruction's own sum is coarser than a chain of fp32 additions: as
// measured on an MI355X (profiles/linear_fp8_numbers.md), a product 2^-14 or
// more below the largest one it is first added to is dropped, and the add
// into the accumulator truncates.  The tests' bound carries a measured
// factor for that.
//
// Quantiser (two passes over the source, fp32 or bf16, optional ReLU mask):
//   amax_kernel   grid-stride max of the |t| bit patterns; every block writes
//                 its own partial, so there is neither an atomic nor a buffer
//                 to clear.
//   cast_kernel   every block reduces the (<= 1024) partials, derives k from
//                 the exponent and mantissa bits, and quantises one 64x64
//                 source tile: a thread owns a 4x4 patch, read as four 4-wide
//                 loads, packed to four dwords and transposed in registers to
//                 four more.  Both sets go to LDS tiles and leave as 16-byte
//                 stores: the row-major copy q[R][pad128(C)] and the
//                 transposed copy qT[C][pad128(R)].  The padding of the
//                 contiguous axis is written as byte 0x00 (+0 in both
//                 formats) by the same blocks, so the GEMM has no k tail.
//                 For gy the tile's fp32 column sums (of the masked,
//                 unquantised values, rows in order) are the partials of gb.
//
// One NT GEMM serves forward, gx and gw:
//     C[m][n] = sum_k A[m][k] * B[n][k],   k contiguous in both operands
//     forward   A = xq   [B][K]        B = wq  [N][K]
//     gx        A = gyq  [B][N] e5m2   B = wqT [K][N]
//     gw        A = gyqT [N][B] e5m2   B = xqT [K][B]
//   - 256 threads as 2x2 waves, 64x64 block tile, 128 bytes of k per LDS
//     tile; a wave owns 32x32 = 2x2 accumulator fragments, so one k tile is
//     four MFMAs of 16x16x128 per wave.
//   - The LDS tiles are double buffered: the next tile's global loads are
//     issued before the MFMAs and stored to the other buffer after them, one
//     barrier per k tile.
//   - A lane's fragment is row (lane & 15), bytes 32*(lane >> 4) .. +31: two
//     16-byte LDS reads.  Rows are 144 bytes apart (36 dwords), so the 16
//     rows that a 16-lane group reads at one byte offset start in 16
//     different 4-bank groups of the 64 banks (36r mod 64 takes every
//     multiple of 4 once for r = 0..15): no conflict.  A and B are both 8-bit
//     and use the same lane -> k mapping, so the sum over k does not depend on
//     which k the hardware assigns to a byte.
//   - B's fragment is the instruction's first operand, so an accumulator
//     holds four consecutive n for one m and leaves as one 8- or 16-byte
//     store into the row-major output.
//   - gw may split its reduction (the batch) over blockIdx.z into a partial
//     buffer that gemm_bf16.h's gw_combine_kernel sums in split order: no
//     float atomics, bitwise reproducible.
//
// K23 — MXFP8: the same GEMM with the instruction's block scales in use.
// A block is 32 consecutive elements along the reduction axis, completed
// with zeros; its scale 2^k follows the rule above from the block's own amax
// and is stored as the e8m0 byte 127 - k of the decode factor 2^-k (in
// [1, 253]).  The instruction multiplies a block's products by both decode
// factors, so the accumulator is the result and the epilogue has no inverse
// scale.
//   mxfp8_quant_kernel  one launch per tensor, no amax pass: the 64x64 tile
//                 of cast_kernel, but every 32-block is scaled on its own.
//                 Along a row the 8 lanes that hold a block exchange their
//                 amax by three xor shuffles.  Along a column a block is 8
//                 thread rows = two waves: two shuffles inside the wave, then
//                 one LDS row per wave.  The transposed copy is cast from the
//                 source with the column scales, so it is not the transpose
//                 of the row copy.  Scale bytes leave as one 16-bit store per
//                 tile row: sq[R][pad128(C)/32], sqT[C][pad128(R)/32].
//                 Padding is byte 0x00 with scale 127, from the same blocks.
//   gemm_fp8_kernel<.., MX>  the instruction scales its k = 32g..32g+31 of
//                 row (lane & 15) by the byte that lane 16g + (lane & 15)
//                 passes, and a lane's two 16-byte register halves are its
//                 k = 16g.. and 64+16g.., g = lane >> 4 (measured:
//                 profiles/linear_mxfp8_numbers.md).  So the MX fragment is
//                 those two 16-byte LDS reads, not 32 consecutive bytes, and
//                 lane group g carries the scale of the row's block g.  The
//                 lane loads that byte of the NEXT k tile straight to a
//                 register together with the operand loads, under the MFMAs;
//                 rows out of range read 127.
//
// Bindings are registered from kernels.hip's PYBIND11_MODULE through
// register_linear_fp8().

#include "gemm_bf16.h"  // cdiv, frag_cd, MAX_DIM, gw_combine_kernel

#include <pybind11/pybind11.h>

#include <algorithm>

namespace {

typedef __attribute__((ext_vector_type(8))) int frag_f8;  // 32 fp8 values

constexpr int TM = 64;             // block tile rows
constexpr int TN = 64;             // block tile cols
constexpr int TK = 128;            // reduction bytes per LDS tile
constexpr int PITCH = TK + 16;     // LDS row pitch in bytes (see above)
constexpr int QT = 64;             // the quantiser's square tile
constexpr int QP = QT / 4 + 4;     // its LDS row pitch in dwords (80 bytes)
constexpr int MAX_AMAX_PART = 1024;
constexpr int WS_SCALE = 2;        // ws = [s, 1/s, amax partials...]

inline int64_t pad128(int64_t n) { return (n + 127) / 128 * 128; }

// ---------------------------------------------------------------------------
// quantiser
// ---------------------------------------------------------------------------
__device__ __forceinline__ float load1(const float* p, int64_t i) {
  return p[i];
}
__device__ __forceinline__ float load1(const bf16_t* p, int64_t i) {
  return to_f(p[i]);
}

// element i of the source, zero where the mask (the saved ReLU output) is
// not positive
template <typename T>
__device__ __forceinline__ float masked1(const T* src, const void* mask,
                                         int mask_f32, int64_t i) {
  const float v = load1(src, i);
  if (!mask) return v;
  const float m = mask_f32 ? ((const float*)mask)[i]
                           : to_f(((const bf16_t*)mask)[i]);
  return m > 0.f ? v : 0.f;
}

// the same for 4 elements from i; the caller guarantees the alignment
template <typename T>
__device__ __forceinline__ void masked4(const T* src, const void* mask,
                                        int mask_f32, int64_t i,
                                        float (&f)[4]) {
  load_vec<T, 4>(src + i, f);
  if (!mask) return;
  float m[4];
  if (mask_f32) load_vec<float, 4>((const float*)mask + i, m);
  else load_vec<bf16_t, 4>((const bf16_t*)mask + i, m);
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (!(m[j] > 0.f)) f[j] = 0.f;
}

// max over the block; every thread gets the result
__device__ __forceinline__ uint32_t block_max(uint32_t v, uint32_t* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, 64));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return max(max(sh[0], sh[1]), max(sh[2], sh[3]));
}

template <typename T>
__global__ __launch_bounds__(BLK) void fp8_amax_kernel(
    const T* __restrict__ src, const void* __restrict__ mask, int mask_f32,
    int64_t n, int vec, uint32_t* __restrict__ part) {
  __shared__ uint32_t sh[NWAVE];
  const int64_t tid = (int64_t)blockIdx.x * BLK + threadIdx.x;
  const int64_t nth = (int64_t)gridDim.x * BLK;
  const int64_t nvec = vec ? n / 4 : 0;
  uint32_t m = 0;
  for (int64_t i = tid; i < nvec; i += nth) {
    float f[4];
    masked4(src, mask, mask_f32, i * 4, f);
#pragma unroll
    for (int j = 0; j < 4; ++j) m = max(m, __float_as_uint(f[j]) & 0x7fffffffu);
  }
  for (int64_t i = nvec * 4 + tid; i < n; i += nth)
    m = max(m, __float_as_uint(masked1(src, mask, mask_f32, i)) & 0x7fffffffu);
  m = block_max(m, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = m;
}

// k of s = 2^k from the bits of amax (finite, sign cleared)
__device__ __forceinline__ int scale_exp(uint32_t amax, int E) {
  if (amax == 0) return 0;
  const int eb = (int)(amax >> 23);
  if (eb == 0) return 126;  // subnormal: E - e > 126 whatever the mantissa
  const int k = E - (eb - 127) - ((amax & 0x7fffffu) > 0x600000u ? 1 : 0);
  return min(126, max(-126, k));
}

template <bool E5M2>
__device__ __forceinline__ uint32_t cvt4(float a, float b, float c, float d) {
  int v = 0;
  if (E5M2) {
    v = __builtin_amdgcn_cvt_pk_bf8_f32(a, b, v, false);
    v = __builtin_amdgcn_cvt_pk_bf8_f32(c, d, v, true);
  } else {
    v = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, v, false);
    v = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, v, true);
  }
  return (uint32_t)v;
}

// grid = (row tiles, col tiles).  q (row pitch ldq) and qT (ldqT) may each
// be null; the grid covers the padded extent of every copy that is wanted.
template <typename T, bool E5M2>
__global__ __launch_bounds__(BLK) void fp8_cast_kernel(
    const T* __restrict__ src, const void* __restrict__ mask, int mask_f32,
    int R, int C, int vec, const uint32_t* __restrict__ amax_part, int n_part,
    float* __restrict__ scale, uint8_t* __restrict__ q, int64_t ldq,
    uint8_t* __restrict__ qT, int64_t ldqT, float* __restrict__ gb_part) {
  __shared__ uint32_t sh[NWAVE];
  __shared__ __attribute__((aligned(16))) uint32_t Qs[QT][QP];
  __shared__ __attribute__((aligned(16))) uint32_t QTs[QT][QP];
  __shared__ float Gs[QT / 4][QT];

  const int tid = threadIdx.x;
  uint32_t amax = 0;
  for (int i = tid; i < n_part; i += BLK) amax = max(amax, amax_part[i]);
  amax = block_max(amax, sh);
  const int k = scale_exp(amax, E5M2 ? 15 : 8);
  const float s = __uint_as_float((uint32_t)(k + 127) << 23);
  if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) {
    scale[0] = s;
    scale[1] = __uint_as_float((uint32_t)(127 - k) << 23);
  }

  const int tx = tid & 15, ty = tid >> 4;
  const int r0 = blockIdx.x * QT + ty * 4, c0 = blockIdx.y * QT + tx * 4;
  uint32_t d[4];
  float cs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = r0 + i;
    float f[4] = {0.f, 0.f, 0.f, 0.f};
    if (r < R) {
      const int64_t at = (int64_t)r * C + c0;
      if (vec && c0 < C) {  // vec: C % 4 == 0, so the 4 are in range
        masked4(src, mask, mask_f32, at, f);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (c0 + j < C) f[j] = masked1(src, mask, mask_f32, at + j);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) cs[j] += f[j];
    d[i] = cvt4<E5M2>(f[0] * s, f[1] * s, f[2] * s, f[3] * s);
    Qs[ty * 4 + i][tx] = d[i];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {  // column c0 + j of the patch, rows r0..r0+3
    const uint32_t t = ((d[0] >> (8 * j)) & 0xffu) |
                       (((d[1] >> (8 * j)) & 0xffu) << 8) |
                       (((d[2] >> (8 * j)) & 0xffu) << 16) |
                       (((d[3] >> (8 * j)) & 0xffu) << 24);
    QTs[tx * 4 + j][ty] = t;
    Gs[ty][tx * 4 + j] = cs[j];
  }
  __syncthreads();

  const int row = tid >> 2, seg = tid & 3;  // 16 bytes of one tile row
  if (q) {
    const int r = blockIdx.x * QT + row;
    if (r < R)
      *reinterpret_cast<uint4*>(q + (int64_t)r * ldq + blockIdx.y * QT +
                                seg * 16) =
          *reinterpret_cast<const uint4*>(&Qs[row][seg * 4]);
  }
  if (qT) {
    const int c = blockIdx.y * QT + row;
    if (c < C)
      *reinterpret_cast<uint4*>(qT + (int64_t)c * ldqT + blockIdx.x * QT +
                                seg * 16) =
          *reinterpret_cast<const uint4*>(&QTs[row][seg * 4]);
  }
  if (gb_part && tid < QT) {
    const int c = blockIdx.y * QT + tid;
    float sum = 0.f;
#pragma unroll
    for (int y = 0; y < QT / 4; ++y) sum += Gs[y][tid];
    if (c < C) gb_part[(int64_t)blockIdx.x * C + c] = sum;
  }
}

// 2^k for one block from its amax bits; byte is the e8m0 code of 2^-k
template <bool E5M2>
__device__ __forceinline__ float mx_scale(uint32_t amax, uint32_t& byte) {
  const int k = scale_exp(amax, E5M2 ? 15 : 8);
  byte = (uint32_t)(127 - k);
  return __uint_as_float((uint32_t)(k + 127) << 23);
}

// K23's quantiser: grid and tile as fp8_cast_kernel.  sq / sqT are the e8m0
// scales of q / qT, ldq / 32 and ldqT / 32 bytes per row.
template <typename T, bool E5M2>
__global__ __launch_bounds__(BLK) void mxfp8_quant_kernel(
    const T* __restrict__ src, const void* __restrict__ mask, int mask_f32,
    int R, int C, int vec, uint8_t* __restrict__ q, uint8_t* __restrict__ sq,
    int64_t ldq, uint8_t* __restrict__ qT, uint8_t* __restrict__ sqT,
    int64_t ldqT, float* __restrict__ gb_part) {
  __shared__ __attribute__((aligned(16))) uint32_t Qs[QT][QP];
  __shared__ __attribute__((aligned(16))) uint32_t QTs[QT][QP];
  __shared__ float Gs[QT / 4][QT];
  __shared__ uint32_t Cm[NWAVE][QT];  // column amax over each wave's 16 rows
  __shared__ __attribute__((aligned(4))) uint8_t Sr[QT][2], Sc[QT][2];

  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4, wave = tid >> 6;
  const int r0 = blockIdx.x * QT + ty * 4, c0 = blockIdx.y * QT + tx * 4;
  float f[4][4];
  uint32_t rm[4] = {0u, 0u, 0u, 0u}, cm[4] = {0u, 0u, 0u, 0u};
  float cs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = r0 + i;
#pragma unroll
    for (int j = 0; j < 4; ++j) f[i][j] = 0.f;
    if (r < R) {
      const int64_t at = (int64_t)r * C + c0;
      if (vec && c0 < C) {  // vec: C % 4 == 0, so the 4 are in range
        masked4(src, mask, mask_f32, at, f[i]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (c0 + j < C) f[i][j] = masked1(src, mask, mask_f32, at + j);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t a = __float_as_uint(f[i][j]) & 0x7fffffffu;
      cs[j] += f[i][j];
      rm[i] = max(rm[i], a);
      cm[j] = max(cm[j], a);
    }
  }

  if (q) {  // a row block is the 8 lanes tx & ~7 .. of one thread row
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int o = 1; o < 8; o <<= 1)
        rm[i] = max(rm[i], (uint32_t)__shfl_xor((int)rm[i], o, 64));
      uint32_t byte;
      const float s = mx_scale<E5M2>(rm[i], byte);
      Qs[ty * 4 + i][tx] =
          cvt4<E5M2>(f[i][0] * s, f[i][1] * s, f[i][2] * s, f[i][3] * s);
      if ((tx & 7) == 0) Sr[ty * 4 + i][tx >> 3] = (uint8_t)byte;
    }
  }
  if (qT) {  // a column block is 8 thread rows: this wave's 4 and its pair's
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      cm[j] = max(cm[j], (uint32_t)__shfl_xor((int)cm[j], 16, 64));
      cm[j] = max(cm[j], (uint32_t)__shfl_xor((int)cm[j], 32, 64));
      if ((ty & 3) == 0) Cm[wave][tx * 4 + j] = cm[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t byte;
      const float s =
          mx_scale<E5M2>(max(cm[j], Cm[wave ^ 1][tx * 4 + j]), byte);
      // column c0 + j of the patch, rows r0..r0+3
      QTs[tx * 4 + j][ty] =
          cvt4<E5M2>(f[0][j] * s, f[1][j] * s, f[2][j] * s, f[3][j] * s);
      if ((ty & 7) == 0) Sc[tx * 4 + j][ty >> 3] = (uint8_t)byte;
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) Gs[ty][tx * 4 + j] = cs[j];
  __syncthreads();

  const int row = tid >> 2, seg = tid & 3;  // 16 bytes of one tile row
  if (q) {
    const int r = blockIdx.x * QT + row;
    if (r < R)
      *reinterpret_cast<uint4*>(q + (int64_t)r * ldq + blockIdx.y * QT +
                                seg * 16) =
          *reinterpret_cast<const uint4*>(&Qs[row][seg * 4]);
    if (tid < QT && blockIdx.x * QT + tid < R)
      *reinterpret_cast<uint16_t*>(sq +
                                   (int64_t)(blockIdx.x * QT + tid) *
                                       (ldq / 32) +
                                   blockIdx.y * 2) =
          *reinterpret_cast<const uint16_t*>(Sr[tid]);
  }
  if (qT) {
    const int c = blockIdx.y * QT + row;
    if (c < C)
      *reinterpret_cast<uint4*>(qT + (int64_t)c * ldqT + blockIdx.x * QT +
                                seg * 16) =
          *reinterpret_cast<const uint4*>(&QTs[row][seg * 4]);
    const int t = tid - QT;  // the second wave writes the scales
    if (t >= 0 && t < QT && blockIdx.y * QT + t < C)
      *reinterpret_cast<uint16_t*>(sqT +
                                   (int64_t)(blockIdx.y * QT + t) *
                                       (ldqT / 32) +
                                   blockIdx.x * 2) =
          *reinterpret_cast<const uint16_t*>(Sc[t]);
  }
  if (gb_part && tid < QT) {
    const int c = blockIdx.y * QT + tid;
    float sum = 0.f;
#pragma unroll
    for (int y = 0; y < QT / 4; ++y) sum += Gs[y][tid];
    if (c < C) gb_part[(int64_t)blockIdx.x * C + c] = sum;
  }
}

// ---------------------------------------------------------------------------
// the GEMM
// ---------------------------------------------------------------------------
struct Fp8Operand {
  const uint8_t* p;        // element (r, k): p[r*ld + k]
  int64_t ld;              // bytes, a multiple of 16; k is padded to 128
  int rows;                // valid r in [0, rows)
  const float* inv_scale;  // 1/s of this tensor, in device memory
  const uint8_t* sc;       // MX: e8m0 block scales, ld / 32 bytes per row
};

// this thread's two 16-byte chunks of the tile rows [r0, r0+64) x bytes
// [k0, k0+128); rows out of range come back as zero
__device__ __forceinline__ void gload(const Fp8Operand& o, int r0, int k0,
                                      int tid, uint4 (&reg)[2]) {
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int c = tid + p * BLK;
    const int r = r0 + (c >> 3);
    reg[p] = r < o.rows
                 ? *reinterpret_cast<const uint4*>(o.p + (int64_t)r * o.ld +
                                                   k0 + (c & 7) * 16)
                 : make_uint4(0u, 0u, 0u, 0u);
  }
}

__device__ __forceinline__ void lstore(uint8_t (*T)[PITCH], int tid,
                                       const uint4 (&reg)[2]) {
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int c = tid + p * BLK;
    *reinterpret_cast<uint4*>(&T[c >> 3][(c & 7) * 16]) = reg[p];
  }
}

// MX: the instruction's k index of a lane's register half h is
// 64*h + 16*(lane >> 4) + byte, and lane group g's scale byte goes to k
// 32*g .. 32*g+31 (measured).  So the lane reads bytes 16*g.. and 64+16*g..
// of its row, and block g of the row is scaled by the byte lane group g holds.
// Without block scales the order within the sum is free and the lane keeps
// its 32 consecutive bytes.
template <bool MX>
__device__ __forceinline__ frag_f8 lfrag(const uint8_t (*T)[PITCH], int row,
                                         int lane) {
  const uint4* p = reinterpret_cast<const uint4*>(
      &T[row + (lane & 15)][(MX ? 16 : 32) * (lane >> 4)]);
  const uint4 lo = p[0], hi = p[MX ? 4 : 1];
  return frag_f8{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w,
                 (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
}

// MX: this lane's scale bytes for its fragments of the tile rows r0 + 16*i,
// k tile k0: row (lane & 15), block (lane >> 4); 127 (2^0) out of range
__device__ __forceinline__ void sload(const Fp8Operand& o, int r0, int k0,
                                      int lane, int (&s)[2]) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r = r0 + i * 16 + (lane & 15);
    s[i] = r < o.rows
               ? (int)o.sc[(int64_t)r * (o.ld >> 5) + (k0 >> 5) + (lane >> 4)]
               : 127;
  }
}

// grid = (m tiles, n tiles, splits); split z reduces the k bytes
// [z*kchunk, min(Kred, (z+1)*kchunk)) into C + z*M*N.  Kred and kchunk are
// multiples of 128.  A is e5m2 if A_E5M2, else e4m3; B is e4m3.  MX: the
// operands carry block scales and no per-tensor inverse scale.
template <bool A_E5M2, bool MX, typename OutT>
__global__ __launch_bounds__(BLK) void gemm_fp8_kernel(
    Fp8Operand A, Fp8Operand B, int Kred, int kchunk, OutT* __restrict__ C,
    const float* __restrict__ bias, int relu, int vec_out) {
  __shared__ __attribute__((aligned(16))) uint8_t As[2][TM][PITCH];
  __shared__ __attribute__((aligned(16))) uint8_t Bs[2][TN][PITCH];

  const int M = A.rows, N = B.rows;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const int m0 = blockIdx.x * TM, n0 = blockIdx.y * TN;
  const int kbeg = blockIdx.z * kchunk;
  const int kend = min(Kred, kbeg + kchunk);

  frag_cd acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = frag_cd{0.f, 0.f, 0.f, 0.f};

  uint4 ra[2], rb[2];
  int sa[2] = {127, 127}, sb[2] = {127, 127}, na[2], nb[2];
  if (kbeg < kend) {
    gload(A, m0, kbeg, tid, ra);
    gload(B, n0, kbeg, tid, rb);
    if constexpr (MX) {
      sload(A, m0 + wm, kbeg, lane, sa);
      sload(B, n0 + wn, kbeg, lane, sb);
    }
    lstore(As[0], tid, ra);
    lstore(Bs[0], tid, rb);
  }
  __syncthreads();
  int buf = 0;
  for (int k0 = kbeg; k0 < kend; k0 += TK, buf ^= 1) {
    const bool more = k0 + TK < kend;
    if (more) {  // next tile's global loads fly under the MFMAs
      gload(A, m0, k0 + TK, tid, ra);
      gload(B, n0, k0 + TK, tid, rb);
      if constexpr (MX) {
        sload(A, m0 + wm, k0 + TK, lane, na);
        sload(B, n0 + wn, k0 + TK, lane, nb);
      }
    }
    frag_f8 a[2], b[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      a[i] = lfrag<MX>(As[buf], wm + i * 16, lane);
      b[i] = lfrag<MX>(Bs[buf], wn + i * 16, lane);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        // B first: the accumulator's 4 registers run along n.  Format
        // selectors: 0 = e4m3, 1 = e5m2; 127 is the block scale 2^0.
        // MX: byte 0 of the lane's scale register, for block lane >> 4.
        if constexpr (MX)
          acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
              b[j], a[i], acc[i][j], 0, A_E5M2 ? 1 : 0, 0, sb[j], 0, sa[i]);
        else
          acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
              b[j], a[i], acc[i][j], 0, A_E5M2 ? 1 : 0, 0, 127, 0, 127);
    if (more) {  // the other buffer was last read before the previous barrier
      lstore(As[buf ^ 1], tid, ra);
      lstore(Bs[buf ^ 1], tid, rb);
      if constexpr (MX) {
#pragma unroll
        for (int i = 0; i < 2; ++i) sa[i] = na[i], sb[i] = nb[i];
      }
    }
    __syncthreads();
  }

  float inv_a = 1.f, inv_b = 1.f;
  if constexpr (!MX) inv_a = *A.inv_scale, inv_b = *B.inv_scale;
  OutT* Cz = C + (int64_t)blockIdx.z * M * N;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int m = m0 + wm + i * 16 + (lane & 15);
      const int n = n0 + wn + j * 16 + (lane >> 4) * 4;
      if (m >= M || n >= N) continue;
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        // two exact multiplications by powers of two: their product alone
        // could leave fp32's range where the result does not
        v[r] = MX ? acc[i][j][r] : acc[i][j][r] * inv_a * inv_b;
        if (bias && n + r < N) v[r] += bias[n + r];
        if (relu) v[r] = fmaxf(v[r], 0.f);
      }
      OutT* dst = Cz + (int64_t)m * N + n;
      if (vec_out && n + 3 < N) {
        store_vec<OutT, 4>(dst, v);
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (n + r < N) from_f(v[r], dst[r]);
      }
    }
}

// ---------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------
static void check_dims(const char* who, std::initializer_list<int64_t> dims) {
  for (int64_t d : dims) {
    if (d < 1)
      throw std::invalid_argument(std::string(who) +
                                  ": every dimension must be >= 1");
    if (pad128(d) > MAX_DIM)
      throw std::invalid_argument(std::string(who) +
                                  ": a dimension does not fit the kernel's "
                                  "32-bit index");
  }
}

static void check_aligned(const char* who,
                          std::initializer_list<uintptr_t> ptrs) {
  for (uintptr_t p : ptrs)
    if (p % 16 != 0)
      throw std::invalid_argument(std::string(who) +
                                  ": fp8 storage, outputs and workspaces "
                                  "must be 16-byte aligned");
}

// bytes per row of a quantised copy whose contiguous axis has n elements
int64_t fp8_pitch(int64_t n) {
  check_dims("fp8_pitch", {n});
  return pad128(n);
}

// floats in the workspace of fp8_quantize: [s, 1/s, amax partials]
int fp8_ws_floats() { return WS_SCALE + MAX_AMAX_PART; }

// Quantise src [R][C] (fp32 or bf16, dense; mask of the same shape, bf16 or
// fp32, 0 = none) to q [R][pitch(C)] and/or qT [C][pitch(R)] (0 = skip).
// ws: fp8_ws_floats() floats; ws[0] = s and ws[1] = 1/s afterwards.
// gb (0 = skip): the fp32 column sums of the masked source, through
// gb_part, a workspace of (pitch(R) / 64) * C floats.
void fp8_quantize(uintptr_t src, bool src_bf16, uintptr_t mask, bool mask_f32,
                  int64_t R, int64_t C, bool e5m2, uintptr_t q, uintptr_t qT,
                  uintptr_t ws, uintptr_t gb_part, uintptr_t gb,
                  uintptr_t stream) {
  check_dims("fp8_quantize", {R, C});
  if (!src || !ws || (!q && !qT))
    throw std::invalid_argument("fp8_quantize: null source, workspace or "
                                "no copy asked for");
  if (gb && !gb_part)
    throw std::invalid_argument("fp8_quantize: gb needs its workspace");
  check_aligned("fp8_quantize", {q, qT, ws, gb_part});
  const int64_t row_tiles = qT ? pad128(R) / QT : cdiv((int)R, QT);
  const int64_t col_tiles = q ? pad128(C) / QT : cdiv((int)C, QT);
  if (col_tiles > 65535)
    throw std::invalid_argument("fp8_quantize: too many columns");
  const int64_t n = R * C;
  const int n_part = (int)std::min<int64_t>(
      MAX_AMAX_PART, (n + (int64_t)BLK * 16 - 1) / ((int64_t)BLK * 16));
  const uintptr_t sb = src_bf16 ? 8 : 16, mb = mask_f32 ? 16 : 8;
  const int vec1 = src % sb == 0 && mask % mb == 0;  // whole tensor, flat
  const int vec2 = vec1 && C % 4 == 0;               // within rows
  float* scale = (float*)ws;
  uint32_t* part = (uint32_t*)(scale + WS_SCALE);
  const dim3 grid((unsigned)row_tiles, (unsigned)col_tiles);
  by_dtype(src_bf16, [&](auto* t) {
    using T = elem_t<decltype(t)>;
    hipLaunchKernelGGL(fp8_amax_kernel<T>, dim3(n_part), dim3(BLK), 0,
                       S(stream), (const T*)src, (const void*)mask,
                       (int)mask_f32, n, vec1, part);
    auto cast = e5m2 ? fp8_cast_kernel<T, true> : fp8_cast_kernel<T, false>;
    hipLaunchKernelGGL(cast, grid, dim3(BLK), 0, S(stream), (const T*)src,
                       (const void*)mask, (int)mask_f32, (int)R, (int)C, vec2,
                       (const uint32_t*)part, n_part, scale, (uint8_t*)q,
                       pad128(C), (uint8_t*)qT, pad128(R),
                       gb ? (float*)gb_part : (float*)nullptr);
  });
  if (gb)
    hipLaunchKernelGGL(gw_combine_kernel, dim3(grid_for(C, BLK)), dim3(BLK), 0,
                       S(stream), (const float*)gb_part, (float*)gb, C,
                       (const float*)nullptr, (float*)nullptr, 0,
                       (int)row_tiles);
}

static Fp8Operand fp8_operand(uintptr_t p, int64_t red, int64_t rows,
                              uintptr_t scale_ws) {
  return Fp8Operand{(const uint8_t*)p, pad128(red), (int)rows,
                    (const float*)scale_ws + 1, nullptr};
}

static Fp8Operand mx_operand(uintptr_t p, uintptr_t sc, int64_t red,
                             int64_t rows) {
  return Fp8Operand{(const uint8_t*)p, pad128(red), (int)rows, nullptr,
                    (const uint8_t*)sc};
}

template <bool A_E5M2, bool MX = false>
static void launch_gemm(const Fp8Operand& a, const Fp8Operand& b, int64_t red,
                        int kchunk, int splits, uintptr_t c, bool out_f32,
                        uintptr_t bias, bool relu, uintptr_t stream) {
  const dim3 grid(cdiv(a.rows, TM), cdiv(b.rows, TN), splits);
  if (grid.y > 65535)
    throw std::invalid_argument("linear_fp8: too many output columns");
  const int vec_out = b.rows % 4 == 0;
  if (out_f32)
    hipLaunchKernelGGL((gemm_fp8_kernel<A_E5M2, MX, float>), grid,
                       dim3(BLK), 0, S(stream), a, b, (int)pad128(red), kchunk,
                       (float*)c, (const float*)bias, (int)relu, vec_out);
  else
    hipLaunchKernelGGL((gemm_fp8_kernel<A_E5M2, MX, bf16_t>), grid,
                       dim3(BLK), 0, S(stream), a, b, (int)pad128(red), kchunk,
                       (bf16_t*)c, (const float*)bias, (int)relu, vec_out);
}

// out[B,N] = (xq[B,K] · wq[N,K]ᵀ) / (sx·sw) (+ bias) (ReLU).  sx, sw: the
// workspaces fp8_quantize left for x and w.
void linear_fp8_fwd(uintptr_t xq, uintptr_t wq, uintptr_t sx, uintptr_t sw,
                    uintptr_t bias, uintptr_t out, int64_t B, int64_t K,
                    int64_t N, bool relu, bool out_f32, uintptr_t stream) {
  check_dims("linear_fp8_fwd", {B, K, N});
  check_aligned("linear_fp8_fwd", {xq, wq, sx, sw, out});
  launch_gemm<false>(fp8_operand(xq, K, B, sx), fp8_operand(wq, K, N, sw), K,
                     (int)pad128(K), 1, out, out_f32, bias, relu, stream);
}

// gx[B,K] = (gyq[B,N] (e5m2) · wqT[K,N]ᵀ) / (sg·sw)
void linear_fp8_bwd_x(uintptr_t gyq, uintptr_t wqT, uintptr_t sg, uintptr_t sw,
                      uintptr_t gx, int64_t B, int64_t K, int64_t N,
                      bool out_f32, uintptr_t stream) {
  check_dims("linear_fp8_bwd_x", {B, K, N});
  check_aligned("linear_fp8_bwd_x", {gyq, wqT, sg, sw, gx});
  launch_gemm<true>(fp8_operand(gyq, N, B, sg), fp8_operand(wqT, N, K, sw), N,
                    (int)pad128(N), 1, gx, out_f32, 0, false, stream);
}

// gemm_bf16.h's gw_split_count rule on this tile: blocks to cover the 256
// CUs twice, each split at least two LDS tiles deep, no empty last split.
int linear_fp8_gw_splits(int64_t B, int64_t K, int64_t N) {
  check_dims("linear_fp8_gw_splits", {B, K, N});
  const int red = (int)pad128(B);
  const int64_t tiles = (int64_t)cdiv((int)N, TM) * cdiv((int)K, TN);
  const int64_t want = (512 + tiles - 1) / tiles;
  const int64_t most = cdiv(red, 2 * TK);
  const int s = (int)std::max<int64_t>(1, std::min(want, most));
  const int kchunk = cdiv(cdiv(red, s), TK) * TK;
  return cdiv(red, kchunk);
}

// gw[N,K] = (gyqT[N,B] (e5m2) · xqT[K,B]ᵀ) / (sg·sx), fp32.
// part: fp32 workspace of splits*N*K floats (unused when splits == 1).
void linear_fp8_bwd_w(uintptr_t gyqT, uintptr_t xqT, uintptr_t sg,
                      uintptr_t sx, uintptr_t gw, uintptr_t part, int splits,
                      int64_t B, int64_t K, int64_t N, uintptr_t stream) {
  check_dims("linear_fp8_bwd_w", {B, K, N});
  if (splits != linear_fp8_gw_splits(B, K, N))
    throw std::invalid_argument("linear_fp8_bwd_w: wrong split count");
  if (splits > 1 && !part)
    throw std::invalid_argument("linear_fp8_bwd_w: no workspace");
  check_aligned("linear_fp8_bwd_w", {gyqT, xqT, sg, sx, gw, part});
  const int kchunk = cdiv(cdiv((int)pad128(B), splits), TK) * TK;
  launch_gemm<true>(fp8_operand(gyqT, B, N, sg), fp8_operand(xqT, B, K, sx), B,
                    kchunk, splits, splits > 1 ? part : gw, true, 0, false,
                    stream);
  if (splits > 1) {
    const int64_t n_gw = N * K;
    hipLaunchKernelGGL(gw_combine_kernel, dim3(grid_for(n_gw, BLK)), dim3(BLK),
                       0, S(stream), (const float*)part, (float*)gw, n_gw,
                       (const float*)nullptr, (float*)nullptr, 0, splits);
  }
}

// ---------------------------------------------------------------------------
// K23 — MXFP8 launchers.  Storage as above; a copy's scales are
// [rows][fp8_pitch(n) / 32] e8m0 bytes.
// ---------------------------------------------------------------------------
// Quantise src [R][C] as fp8_quantize does, every 32-block with its own
// scale: q, sq blocked along C; qT, sqT blocked along R (0 = skip a copy).
void mxfp8_quantize(uintptr_t src, bool src_bf16, uintptr_t mask,
                    bool mask_f32, int64_t R, int64_t C, bool e5m2,
                    uintptr_t q, uintptr_t sq, uintptr_t qT, uintptr_t sqT,
                    uintptr_t gb_part, uintptr_t gb, uintptr_t stream) {
  check_dims("mxfp8_quantize", {R, C});
  if (!src || (!q && !qT) || !q != !sq || !qT != !sqT)
    throw std::invalid_argument("mxfp8_quantize: null source, no copy asked "
                                "for, or a copy without its scales");
  if (gb && !gb_part)
    throw std::invalid_argument("mxfp8_quantize: gb needs its workspace");
  check_aligned("mxfp8_quantize", {q, sq, qT, sqT, gb_part});
  const int64_t row_tiles = qT ? pad128(R) / QT : cdiv((int)R, QT);
  const int64_t col_tiles = q ? pad128(C) / QT : cdiv((int)C, QT);
  if (col_tiles > 65535)
    throw std::invalid_argument("mxfp8_quantize: too many columns");
  const uintptr_t sb = src_bf16 ? 8 : 16, mb = mask_f32 ? 16 : 8;
  const int vec = src % sb == 0 && mask % mb == 0 && C % 4 == 0;
  const dim3 grid((unsigned)row_tiles, (unsigned)col_tiles);
  by_dtype(src_bf16, [&](auto* t) {
    using T = elem_t<decltype(t)>;
    auto quant =
        e5m2 ? mxfp8_quant_kernel<T, true> : mxfp8_quant_kernel<T, false>;
    hipLaunchKernelGGL(quant, grid, dim3(BLK), 0, S(stream), (const T*)src,
                       (const void*)mask, (int)mask_f32, (int)R, (int)C, vec,
                       (uint8_t*)q, (uint8_t*)sq, pad128(C), (uint8_t*)qT,
                       (uint8_t*)sqT, pad128(R),
                       gb ? (float*)gb_part : (float*)nullptr);
  });
  if (gb)
    hipLaunchKernelGGL(gw_combine_kernel, dim3(grid_for(C, BLK)), dim3(BLK), 0,
                       S(stream), (const float*)gb_part, (float*)gb, C,
                       (const float*)nullptr, (float*)nullptr, 0,
                       (int)row_tiles);
}

// out[B,N] = sum over K blocks of (xq · wqᵀ) 2^(sx-127) 2^(sw-127) (+ bias)
// (ReLU); sx [B][pitch(K)/32], sw [N][pitch(K)/32]
void linear_mxfp8_fwd(uintptr_t xq, uintptr_t wq, uintptr_t sx, uintptr_t sw,
                      uintptr_t bias, uintptr_t out, int64_t B, int64_t K,
                      int64_t N, bool relu, bool out_f32, uintptr_t stream) {
  check_dims("linear_mxfp8_fwd", {B, K, N});
  check_aligned("linear_mxfp8_fwd", {xq, wq, sx, sw, out});
  launch_gemm<false, true>(mx_operand(xq, sx, K, B), mx_operand(wq, sw, K, N),
                           K, (int)pad128(K), 1, out, out_f32, bias, relu,
                           stream);
}

// gx[B,K] from gyq[B,N] (e5m2) and wqT[K,N], both blocked along N
void linear_mxfp8_bwd_x(uintptr_t gyq, uintptr_t wqT, uintptr_t sg,
                        uintptr_t swT, uintptr_t gx, int64_t B, int64_t K,
                        int64_t N, bool out_f32, uintptr_t stream) {
  check_dims("linear_mxfp8_bwd_x", {B, K, N});
  check_aligned("linear_mxfp8_bwd_x", {gyq, wqT, sg, swT, gx});
  launch_gemm<true, true>(mx_operand(gyq, sg, N, B),
                          mx_operand(wqT, swT, N, K), N, (int)pad128(N), 1, gx,
                          out_f32, 0, false, stream);
}

// gw[N,K] (fp32) from gyqT[N,B] (e5m2) and xqT[K,B], both blocked along B;
// splits and part as linear_fp8_bwd_w.  A split's chunk is a multiple of
// 128 bytes, so no block straddles two splits.
void linear_mxfp8_bwd_w(uintptr_t gyqT, uintptr_t xqT, uintptr_t sgT,
                        uintptr_t sxT, uintptr_t gw, uintptr_t part,
                        int splits, int64_t B, int64_t K, int64_t N,
                        uintptr_t stream) {
  check_dims("linear_mxfp8_bwd_w", {B, K, N});
  if (splits != linear_fp8_gw_splits(B, K, N))
    throw std::invalid_argument("linear_mxfp8_bwd_w: wrong split count");
  if (splits > 1 && !part)
    throw std::invalid_argument("linear_mxfp8_bwd_w: no workspace");
  check_aligned("linear_mxfp8_bwd_w", {gyqT, xqT, sgT, sxT, gw, part});
  const int kchunk = cdiv(cdiv((int)pad128(B), splits), TK) * TK;
  launch_gemm<true, true>(mx_operand(gyqT, sgT, B, N),
                          mx_operand(xqT, sxT, B, K), B, kchunk, splits,
                          splits > 1 ? part : gw, true, 0, false, stream);
  if (splits > 1) {
    const int64_t n_gw = N * K;
    hipLaunchKernelGGL(gw_combine_kernel, dim3(grid_for(n_gw, BLK)), dim3(BLK),
                       0, S(stream), (const float*)part, (float*)gw, n_gw,
                       (const float*)nullptr, (float*)nullptr, 0, splits);
  }
}

}  // namespace

void register_linear_fp8(pybind11::module_& m) {
  m.def("fp8_pitch", &fp8_pitch);
  m.def("fp8_ws_floats", &fp8_ws_floats);
  m.def("fp8_quantize", &fp8_quantize);
  m.def("linear_fp8_fwd", &linear_fp8_fwd);
  m.def("linear_fp8_bwd_x", &linear_fp8_bwd_x);
  m.def("linear_fp8_gw_splits", &linear_fp8_gw_splits);
  m.def("linear_fp8_bwd_w", &linear_fp8_bwd_w);
  m.def("mxfp8_quantize", &mxfp8_quantize);
  m.def("linear_mxfp8_fwd", &linear_mxfp8_fwd);
  m.def("linear_mxfp8_bwd_x", &linear_mxfp8_bwd_x);
  m.def("linear_mxfp8_bwd_w", &linear_mxfp8_bwd_w);
}
