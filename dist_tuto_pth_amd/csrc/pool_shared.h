// pool_shared.h — what pool.hip (NCHW) and pool_nhwc.hip (channels-last)
// share: the division-free index arithmetic (FastDiv, PlanePos), the
// max-pool geometry and its guards (PoolGeom, pool_geom), and the guards
// and the lane count of the global average pool.  One definition each.
#pragma once

#include "common.h"

// n / d for 0 <= n < 2^31 and 1 <= d <= 2^29 without a hardware division
// (Granlund and Montgomery's multiply and shift, rounded-up multiplier):
// with s = ceil(log2 d) and m = floor(2^32 * (2^s - d) / d) + 1,
// n / d = (mulhi(n, m) + n) >> s.  The element-index divisions are most of
// the arithmetic of the pool kernels, which are otherwise a few loads.
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

// planes are indexed in 32 bits; the bound leaves room for the padded and
// strided forms of the index ((H+1)*(W+1) outputs, hp + sh) in an int
constexpr int64_t POOL_MAX_PLANE = (int64_t)1 << 29;
constexpr int64_t POOL_MAX_ELEMS = (int64_t)1 << 62;

inline PoolGeom pool_geom(const char* who, int64_t B, int64_t C, int64_t H,
                          int64_t W, int64_t kh, int64_t kw, int64_t sh,
                          int64_t sw, int64_t ph, int64_t pw) {
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
  if (H * W > POOL_MAX_PLANE || sh > POOL_MAX_PLANE || sw > POOL_MAX_PLANE ||
      B * C > POOL_MAX_ELEMS / (H * W))
    throw std::invalid_argument(op + ": too many elements");
  PoolGeom g;
  g.H = (int)H; g.W = (int)W; g.OH = (int)OH; g.OW = (int)OW;
  g.kh = (int)kh; g.kw = (int)kw; g.sh = (int)sh; g.sw = (int)sw;
  g.ph = (int)ph; g.pw = (int)pw;
  g.by_W = FastDiv((uint32_t)W); g.by_OW = FastDiv((uint32_t)OW);
  g.by_sh = FastDiv((uint32_t)sh); g.by_sw = FastDiv((uint32_t)sw);
  return g;
}

inline void check_gap(const char* who, int64_t planes, int64_t HW,
                      uintptr_t a, uintptr_t b) {
  const std::string op(who);
  if (planes < 1 || HW < 1)
    throw std::invalid_argument(op + ": B*C and H*W must be >= 1");
  if (HW > POOL_MAX_PLANE || planes > POOL_MAX_ELEMS / HW)
    throw std::invalid_argument(op + ": too many elements");
  if (!a || !b) throw std::invalid_argument(op + ": null tensor");
}

// lanes that share one plane's sum in the global average pool: a power of
// two in 1..64 from H*W alone, about four elements per lane
inline int gap_lanes(int64_t HW) {
  int L = 1;
  while (L < 64 && (int64_t)L * 4 < HW) L *= 2;
  return L;
}
