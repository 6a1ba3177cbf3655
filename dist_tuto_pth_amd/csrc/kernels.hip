// kernels.hip — hand-written CDNA4 (gfx950/MI355X) kernels for the fp32
// ops of the reference training path (K1/K2 conv, K7/K8
// linear, K9/K10 log_softmax and NLL, K11-K13 SGD) plus the
// local-reduction primitives of the hand-rolled ring all-reduce (K14).
// The pointwise and pooling ops (K3-K6) live in pointwise.hip.
//
// The reference gets these ops implicitly from torch
// (Net.forward train_dist.py:64-71, SGD train_dist.py:110,124); here
// each is an explicit HIP kernel designed for CDNA4: 64-wide wavefronts,
// 256-thread blocks, 16-byte global access where layout permits
// (vec_sweep), LDS staging of the conv/linear weights, grid-stride
// loops capped so the 256-CU chip is filled without launch spam.
//
// fp32 throughout (the reference trains fp32); bf16 enters for the
// ring-allreduce reduction path (BASELINE config 5), as bf16_t with its
// arithmetic in fp32 like every other bf16 path (common.h).
// Build: hipcc --offload-arch=gfx950 (build.py).  No CUDA paths.
//
// This file also owns PYBIND11_MODULE; each other translation unit
// registers its bindings through the register_*() function declared in
// front of the module.

#include "common.h"

#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <vector>

namespace {

// ===========================================================================
// Weight staging for conv2d and linear.  A weight tensor of at most 64 KB
// is copied into the dynamic LDS buffer once per block and read from
// there; a larger one is read from global memory, where it is L2-hot and
// shared by every block.  stage_for() decides on the host and
// stage_weights() acts on it in the kernel.
// ===========================================================================
struct Staging {
  int staged;
  int lds_bytes;
};

Staging stage_for(int64_t nfloats) {
  const int64_t need = nfloats * sizeof(float);
  if (need <= 64 * 1024) return {1, (int)need};  // LDS budget per block
  return {0, 0};
}

// where to read the n floats of w from; every thread of the block calls it
__device__ __forceinline__ const float* stage_weights(const float* w, int n,
                                                      int staged) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  if (!staged) return w;
  for (int i = threadIdx.x; i < n; i += blockDim.x) smem[i] = w[i];
  __syncthreads();
  return smem;
}

// ===========================================================================
// K1/K2 — direct convolution, stride 1, no padding (the only form Net
// uses: 5x5 kernels, C in {1,10}, K in {10,20}, H<=28).
// One thread per output element across the whole tensor, grid-stride:
// that fills the 256-CU chip at any batch size (a block per batch element
// left half the chip idle at B=128).  The weights come through
// stage_weights(); x is read from global memory, tiny and L2-resident.
// ===========================================================================
__global__ void conv2d_fwd_kernel(const float* __restrict__ x,
                                  const float* __restrict__ w,
                                  const float* __restrict__ bias,
                                  float* __restrict__ out,
                                  int B, int C, int H, int W,
                                  int K, int R, int S_, int staged) {
  const int OH = H - R + 1, OW = W - S_ + 1;
  const float* ws = stage_weights(w, K * C * R * S_, staged);

  const int64_t n_out = (int64_t)B * K * OH * OW;
  const int xn = C * H * W;
  const int on = K * OH * OW;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i < n_out; i += (int64_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / on);
    const int k = (int)((i / (OH * OW)) % K);
    const int oh = (int)((i / OW) % OH);
    const int ow = (int)(i % OW);
    float acc = bias ? bias[k] : 0.f;
    const float* xb = x + (int64_t)b * xn;
    const float* wk = ws + k * C * R * S_;
    for (int c = 0; c < C; ++c) {
      const float* xc = xb + c * H * W + oh * W + ow;
      const float* wc = wk + c * R * S_;
      #pragma unroll 5
      for (int r = 0; r < R; ++r) {
        const float* xrow = xc + r * W;
        const float* wrow = wc + r * S_;
        float a = 0.f;
        #pragma unroll 5
        for (int s = 0; s < S_; ++s) a += xrow[s] * wrow[s];
        acc += a;
      }
    }
    out[i] = acc;
  }
}

// backward dx: gx[b,c,h,w] = sum_k sum_{r,s} gy[b,k,h-r,w-s] * w[k,c,r,s]
// (valid range only).  One thread per gx element, grid-stride; the weights
// come through stage_weights(), gy is read from global memory.
__global__ void conv2d_bwd_x_kernel(const float* __restrict__ gy,
                                    const float* __restrict__ w,
                                    float* __restrict__ gx,
                                    int B, int C, int H, int W,
                                    int K, int R, int S_, int staged) {
  const int OH = H - R + 1, OW = W - S_ + 1;
  const float* ws = stage_weights(w, K * C * R * S_, staged);

  const int64_t n_in = (int64_t)B * C * H * W;
  const int xn = C * H * W;
  const int gn = K * OH * OW;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i < n_in; i += (int64_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / xn);
    const int c = (int)((i / (H * W)) % C);
    const int h = (int)((i / W) % H);
    const int wcol = (int)(i % W);
    const float* gb = gy + (int64_t)b * gn;
    float acc = 0.f;
    const int r0 = max(0, h - OH + 1), r1 = min(R, h + 1);
    const int s0 = max(0, wcol - OW + 1), s1 = min(S_, wcol + 1);
    for (int k = 0; k < K; ++k) {
      const float* gk = gb + k * OH * OW;
      const float* wk = ws + (k * C + c) * R * S_;
      for (int r = r0; r < r1; ++r) {
        const int oh = h - r;
        const float* grow = gk + oh * OW + wcol;
        const float* wrow = wk + r * S_;
        float a = 0.f;
        for (int s = s0; s < s1; ++s) a += grow[-s] * wrow[s];
        acc += a;
      }
    }
    gx[i] = acc;
  }
}

// backward dw/db on a grid of (weight tiles, batch chunks): a thread owns
// one gw (or gb) element and sums its chunk's batch elements in a register.
// With one chunk it stores the sum; with more it adds it atomically into
// gw/gb, which split_batch() zeroed.
__global__ void conv2d_bwd_w_kernel(const float* __restrict__ x,
                                    const float* __restrict__ gy,
                                    float* __restrict__ gw,
                                    float* __restrict__ gb,
                                    int B, int C, int H, int W,
                                    int K, int R, int S_, int bchunk) {
  const int OH = H - R + 1, OW = W - S_ + 1;
  const int xn = C * H * W;
  const int gn = K * OH * OW;
  const int wn = K * C * R * S_;
  const int nchunks = (B + bchunk - 1) / bchunk;
  const int chunk = blockIdx.y;
  const int b0 = chunk * bchunk;
  const int b1 = min(B, b0 + bchunk);

  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < wn;
       i += gridDim.x * blockDim.x) {
    const int k = i / (C * R * S_);
    const int c = (i / (R * S_)) % C;
    const int r = (i / S_) % R;
    const int sx = i % S_;
    float acc = 0.f;
    for (int b = b0; b < b1; ++b) {
      const float* gk = gy + (int64_t)b * gn + k * OH * OW;
      const float* xc = x + (int64_t)b * xn + c * H * W + r * W + sx;
      for (int oh = 0; oh < OH; ++oh) {
        const float* grow = gk + oh * OW;
        const float* xrow = xc + oh * W;
        float a = 0.f;
        for (int ow = 0; ow < OW; ++ow) a += grow[ow] * xrow[ow];
        acc += a;
      }
    }
    if (nchunks == 1) gw[i] = acc;
    else atomicAdd(&gw[i], acc);
  }
  if (gb) {
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < K;
         k += gridDim.x * blockDim.x) {
      float acc = 0.f;
      for (int b = b0; b < b1; ++b) {
        const float* gk = gy + (int64_t)b * gn + k * OH * OW;
        for (int i2 = 0; i2 < OH * OW; ++i2) acc += gk[i2];
      }
      if (nchunks == 1) gb[k] = acc;
      else atomicAdd(&gb[k], acc);
    }
  }
}

// ===========================================================================
// K7/K8 — linear: out[B,N] = x[B,K] @ w[N,K]^T + bias, optional fused
// ReLU epilogue (fc1, train_dist.py:68).  Net shapes (K=320,N=50 and
// K=50,N=10) are tiny: the whole weight panel fits LDS, each block
// stages w once and sweeps a stripe of batch rows; x rows are read
// once, each thread owning one (b,n) output.
// ===========================================================================
__global__ void linear_fwd_kernel(const float* __restrict__ x,
                                  const float* __restrict__ w,
                                  const float* __restrict__ bias,
                                  float* __restrict__ out,
                                  int B, int K, int N, int fuse_relu,
                                  int staged) {
  const float* ws = stage_weights(w, N * K, staged);

  const int64_t n_out = (int64_t)B * N;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i < n_out; i += (int64_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / N);
    const int n = (int)(i % N);
    const float* xr = x + (int64_t)b * K;
    const float* wr = ws + n * K;
    float acc = bias ? bias[n] : 0.f;
    int k = 0;
    for (; k + 4 <= K; k += 4)
      acc += xr[k] * wr[k] + xr[k + 1] * wr[k + 1] +
             xr[k + 2] * wr[k + 2] + xr[k + 3] * wr[k + 3];
    for (; k < K; ++k) acc += xr[k] * wr[k];
    if (fuse_relu && acc < 0.f) acc = 0.f;
    out[i] = acc;
  }
}

// gx[B,K] = gy'[B,N] @ w[N,K]  (gy' = gy masked by out>0 when fused)
__global__ void linear_bwd_x_kernel(const float* __restrict__ gy,
                                    const float* __restrict__ out,
                                    const float* __restrict__ w,
                                    float* __restrict__ gx,
                                    int B, int K, int N, int staged) {
  const float* ws = stage_weights(w, N * K, staged);

  const int64_t n_out = (int64_t)B * K;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i < n_out; i += (int64_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / K);
    const int k = (int)(i % K);
    const float* gr = gy + (int64_t)b * N;
    const float* orow = out ? out + (int64_t)b * N : nullptr;
    float acc = 0.f;
    for (int n = 0; n < N; ++n) {
      float g = gr[n];
      if (orow && orow[n] <= 0.f) g = 0.f;
      acc += g * ws[n * K + k];
    }
    gx[i] = acc;
  }
}

// gw[N,K] += sum_b gy'[b,n] * x[b,k] ; gb[N] += sum_b gy'[b,n]
// Each block owns a batch stripe, accumulates partials, atomically adds.
__global__ void linear_bwd_w_kernel(const float* __restrict__ x,
                                    const float* __restrict__ gy,
                                    const float* __restrict__ out,
                                    float* __restrict__ gw,
                                    float* __restrict__ gb,
                                    int B, int K, int N, int bchunk) {
  const int nchunks = (B + bchunk - 1) / bchunk;
  const int b0 = blockIdx.y * bchunk;
  const int b1 = min(B, b0 + bchunk);
  const int wn = N * K;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < wn;
       i += gridDim.x * blockDim.x) {
    const int n = i / K;
    const int k = i % K;
    float acc = 0.f;
    for (int b = b0; b < b1; ++b) {
      float g = gy[(int64_t)b * N + n];
      if (out && out[(int64_t)b * N + n] <= 0.f) g = 0.f;
      acc += g * x[(int64_t)b * K + k];
    }
    if (nchunks == 1) gw[i] = acc;
    else atomicAdd(&gw[i], acc);
  }
  if (gb) {
    for (int n = blockIdx.x * blockDim.x + threadIdx.x; n < N;
         n += gridDim.x * blockDim.x) {
      float acc = 0.f;
      for (int b = b0; b < b1; ++b) {
        float g = gy[(int64_t)b * N + n];
        if (out && out[(int64_t)b * N + n] <= 0.f) g = 0.f;
        acc += g;
      }
      if (nchunks == 1) gb[n] = acc;
      else atomicAdd(&gb[n], acc);
    }
  }
}

// ===========================================================================
// K9/K10 — log_softmax over dim 1 (train_dist.py:71) and NLL loss
// (train_dist.py:120), plus the fused single-pass form.
// N is tiny (10): one thread per row, serial max/sum over N — the
// tensor is L2-resident at these sizes and the op is launch-bound.
// ===========================================================================
// one row: orow = xr - logsumexp(xr)
__device__ __forceinline__ void log_softmax_row(const float* xr, float* orow,
                                                int N) {
  float m = xr[0];
  for (int i = 1; i < N; ++i) m = fmaxf(m, xr[i]);
  float s = 0.f;
  for (int i = 0; i < N; ++i) s += __expf(xr[i] - m);
  const float lse = m + __logf(s);
  for (int i = 0; i < N; ++i) orow[i] = xr[i] - lse;
}

__global__ void log_softmax_fwd_kernel(const float* __restrict__ x,
                                       float* __restrict__ out,
                                       int B, int N) {
  for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < B;
       b += (int64_t)gridDim.x * blockDim.x)
    log_softmax_row(x + b * N, out + b * N, N);
}

// gx = gy - exp(out) * sum(gy)
__global__ void log_softmax_bwd_kernel(const float* __restrict__ gy,
                                       const float* __restrict__ out,
                                       float* __restrict__ gx,
                                       int B, int N) {
  for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < B;
       b += (int64_t)gridDim.x * blockDim.x) {
    const float* gr = gy + b * N;
    const float* orow = out + b * N;
    float s = 0.f;
    for (int i = 0; i < N; ++i) s += gr[i];
    for (int i = 0; i < N; ++i)
      gx[b * N + i] = gr[i] - __expf(orow[i]) * s;
  }
}

// The two loss kernels add their block's share of the mean into *loss
// (zeroed by the launcher): block_sum needs the BLK threads they are
// launched with.
__global__ __launch_bounds__(BLK) void nll_loss_fwd_kernel(
    const float* __restrict__ logp, const int64_t* __restrict__ target,
    float* __restrict__ loss, int B, int N) {
  __shared__ float sh[NWAVE];
  float acc = 0.f;
  for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < B;
       b += (int64_t)gridDim.x * blockDim.x)
    acc -= logp[b * N + target[b]];
  const float sum = block_sum(acc, sh);
  if (threadIdx.x == 0) atomicAdd(loss, sum / B);
}

// gloss arrives as a DEVICE scalar pointer so the whole backward is
// hipGraph-capturable (no host read of the grad seed).
__global__ void nll_loss_bwd_kernel(const int64_t* __restrict__ target,
                                    float* __restrict__ gx,
                                    const float* __restrict__ gloss,
                                    int B, int N) {
  const float sc = -gloss[0] / B;
  for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < B;
       b += (int64_t)gridDim.x * blockDim.x)
    gx[b * N + target[b]] = sc;
}

// fused: logp + mean NLL in one pass (K9+K10)
__global__ __launch_bounds__(BLK) void log_softmax_nll_fwd_kernel(
    const float* __restrict__ x, const int64_t* __restrict__ tgt,
    float* __restrict__ logp, float* __restrict__ loss, int B, int N) {
  __shared__ float sh[NWAVE];
  float acc = 0.f;
  for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < B;
       b += (int64_t)gridDim.x * blockDim.x) {
    float* lr = logp + b * N;
    log_softmax_row(x + b * N, lr, N);
    acc -= lr[tgt[b]];
  }
  const float sum = block_sum(acc, sh);
  if (threadIdx.x == 0) atomicAdd(loss, sum / B);
}

// gx = (exp(logp) - onehot) * gloss / B
__global__ void log_softmax_nll_bwd_kernel(const float* __restrict__ logp,
                                           const int64_t* __restrict__ tgt,
                                           float* __restrict__ gx,
                                           const float* __restrict__ gloss,
                                           int B, int N) {
  const float sc = gloss[0] / B;
  for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < B;
       b += (int64_t)gridDim.x * blockDim.x) {
    const float* lr = logp + b * N;
    float* gr = gx + b * N;
    const int64_t t = tgt[b];
    for (int i = 0; i < N; ++i)
      gr[i] = (__expf(lr[i]) - (i == t ? 1.f : 0.f)) * sc;
  }
}

// ===========================================================================
// K11-K13 — fused multi-tensor SGD+momentum: buf = mu*buf + g;
// p -= lr*buf; optionally g = 0 (K12 folded in).  All of Net's 8
// tensors in ONE launch: pointer table passed by value.
// Two compile-time options follow torch's rule: weight decay (WD) takes
// g' = g + wd*p for g, Nesterov momentum (NEST) steps along g' + mu*buf
// instead of buf.  The <false, false> instance is the arithmetic above and
// nothing else.
// ===========================================================================
#define MT_MAX 32
struct MtArgs {
  float* p[MT_MAX];
  float* g[MT_MAX];
  float* buf[MT_MAX];
  int64_t numel[MT_MAX];
  int64_t offset[MT_MAX];  // prefix sum for flat indexing
  int count;
  int64_t total;
};

template <bool WD, bool NEST>
__global__ void sgd_step_kernel(MtArgs a, float lr, float mu, float wd,
                                int zero_grad) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i < a.total; i += (int64_t)gridDim.x * blockDim.x) {
    // binary search the tensor containing flat index i
    int lo = 0, hi = a.count - 1;
    while (lo < hi) {
      int mid = (lo + hi + 1) >> 1;
      if (i >= a.offset[mid]) lo = mid; else hi = mid - 1;
    }
    const int64_t j = i - a.offset[lo];
    float g = a.g[lo][j];
    if (WD) g = g + wd * a.p[lo][j];
    if (NEST) {
      // the wrapper refuses Nesterov without momentum: buf is never null
      const float b = mu * a.buf[lo][j] + g;
      a.buf[lo][j] = b;
      g = g + mu * b;
    } else if (a.buf[lo]) {
      g = mu * a.buf[lo][j] + g;
      a.buf[lo][j] = g;
    }
    a.p[lo][j] -= lr * g;
    if (zero_grad) a.g[lo][j] = 0.f;
  }
}

// ===========================================================================
// K14 helpers — local reductions for the hand-rolled / hand-tuned ring
// all-reduce (allreduce.py:26,31 corrected): dst += src, vectorized.
// fp32 and bf16 (BASELINE config 5).
//
// MFMA considered and rejected for this op: a column reduction is
// out[j] = sum_p src[p][j], i.e. ones[1xP] x src[PxN].  On a 16x16x4
// f32 MFMA every C row would hold the same 4-row partial sum, so one
// 4-cycle instruction reduces 4x16 = 64 elements = 16 elem/cycle/wave,
// while plain VALU v_add_f32 reduces 64 elem/cycle/wave — the matrix
// pipe wastes a 16x output replication on a rank-1 operand.  The op is
// HBM-bandwidth-bound anyway (reads P*N floats once); the 16-byte
// grid-stride form below saturates that.  MFMA belongs to GEMM-shaped
// work, which this framework's models reach through the register-
// blocked conv kernels above (shapes are 5x5/latency-bound, below the
// MFMA payoff threshold) and hipBLASLt/MIOpen for ResNet-50.
//
// Each kernel is one vec_sweep (common.h) over T = float or bf16_t: 16
// bytes per lane, then a scalar tail, every sum and product in fp32 and
// one rounding to T at the store.
// ===========================================================================

// The store of the two reductions.  fp32 is store_vec.  bf16 rounds with
// the compiler's fp32 -> bf16 conversion (to nearest even, one
// v_cvt_pk_bf16_f32 per pair on gfx950) where store_vec's f2bf is five
// integer operations per element: measured at 16M elements, f2bf put
// add_inplace 5 % and reduce_columns 1 % outside the run-to-run range of the
// kernels this replaces.  A NaN keeps the bits the hardware gives it.
template <int V>
__device__ __forceinline__ void store_sum(float* p, const float (&f)[V]) {
  store_vec<float, V>(p, f);
}
template <int V>
__device__ __forceinline__ void store_sum(bf16_t* p, const float (&f)[V]) {
  Vec<bf16_t, V> u;
#pragma unroll
  for (int j = 0; j < V; ++j)
    u.e[j] = __builtin_bit_cast(bf16_t, static_cast<__bf16>(f[j]));
  *reinterpret_cast<typename Raw<sizeof(bf16_t) * V>::type*>(p) = u.raw;
}

template <typename T>
__global__ __launch_bounds__(BLK) void add_inplace_kernel(
    T* __restrict__ dst, const T* __restrict__ src, int64_t n) {
  vec_sweep<T>(n, [=](int64_t i, auto width) {
    constexpr int V = decltype(width)::value;
    float a[V], b[V];
    load_vec<T, V>(dst + i, a);
    load_vec<T, V>(src + i, b);
#pragma unroll
    for (int j = 0; j < V; ++j) a[j] += b[j];
    store_sum<V>(dst + i, a);
  });
}

// column reduction for the full-mesh reduce-scatter (K14): after the
// grouped p2p exchange, rank i holds P-1 peer chunks contiguously in
// scratch; one kernel folds them all into the owned chunk.
// dst[j] = (dst[j] + sum_p src[p*stride + j]) * scale, summed in the order
// dst, p = 0..P-1.  bf16 so accumulates in fp32 and rounds ONCE at the end
// (better than serial bf16 adds — BASELINE config 5 accuracy note,
// SURVEY.md §7 hard part d).  The launcher checks that stride keeps every
// row's 16-byte accesses aligned.
template <typename T>
__global__ __launch_bounds__(BLK) void reduce_columns_kernel(
    T* __restrict__ dst, const T* __restrict__ src, int P, int64_t stride,
    int64_t n, float scale) {
  vec_sweep<T>(n, [=](int64_t i, auto width) {
    constexpr int V = decltype(width)::value;
    float a[V], b[V];
    load_vec<T, V>(dst + i, a);
    for (int p = 0; p < P; ++p) {
      load_vec<T, V>(src + p * stride + i, b);
#pragma unroll
      for (int j = 0; j < V; ++j) a[j] += b[j];
    }
#pragma unroll
    for (int j = 0; j < V; ++j) a[j] *= scale;
    store_sum<V>(dst + i, a);
  });
}

__global__ __launch_bounds__(BLK) void scale_f32_kernel(
    float* __restrict__ dst, float s, int64_t n) {
  vec_sweep<float>(n, [=](int64_t i, auto width) {
    constexpr int V = decltype(width)::value;
    float a[V];
    load_vec<float, V>(dst + i, a);
#pragma unroll
    for (int j = 0; j < V; ++j) a[j] *= s;
    store_vec<float, V>(dst + i, a);
  });
}

// grid-throttled 16-byte copy: a stand-in for a link-bound transfer in
// single-GPU overlap probes.  RCCL moves an xGMI peer copy with a few
// workgroups at ~153 GB/s per link — a full-rate DtoD memcpy (5+ TB/s,
// all of HBM) is the WRONG model for it.  Limiting the grid caps the
// copy's HBM draw so the concurrent reduce kernel has headroom, which
// is exactly the real pipeline's situation.
__global__ __launch_bounds__(BLK) void copy_throttled_f32_kernel(
    float* __restrict__ dst, const float* __restrict__ src, int64_t n) {
  vec_sweep<float>(n, [=](int64_t i, auto width) {
    constexpr int V = decltype(width)::value;
    float v[V];
    load_vec<float, V>(src + i, v);
    store_vec<float, V>(dst + i, v);
  });
}

// ===========================================================================
// host launchers + pybind
// ===========================================================================

void conv2d_fwd(uintptr_t x, uintptr_t w, uintptr_t bias, uintptr_t out,
                int B, int C, int H, int W, int K, int R, int S_,
                uintptr_t stream) {
  const Staging st = stage_for((int64_t)K * C * R * S_);
  const int OH = H - R + 1, OW = W - S_ + 1;
  const int64_t n = (int64_t)B * K * OH * OW;
  hipLaunchKernelGGL(conv2d_fwd_kernel, dim3(grid_for(n, BLK)), dim3(BLK),
                     st.lds_bytes, S(stream), (const float*)x,
                     (const float*)w, (const float*)bias, (float*)out, B,
                     C, H, W, K, R, S_, st.staged);
}

// The weight-gradient kernels of conv2d and linear run on a grid of
// (wtiles, nchunks): wn weights in tiles of BLK, the batch in chunks of
// bchunk, halved until the grid has about 512 blocks.  More than one chunk
// accumulates atomically, so gw[wn] and gb[nb] (if any) are zeroed first.
struct BatchSplit {
  int wtiles, bchunk, nchunks;
};

BatchSplit split_batch(int B, int wn, uintptr_t gw, uintptr_t gb, int nb,
                       uintptr_t stream) {
  BatchSplit s{(wn + BLK - 1) / BLK, B, 1};
  while (s.bchunk > 1 && s.wtiles * ((B + s.bchunk - 1) / s.bchunk) < 512)
    s.bchunk = (s.bchunk + 1) / 2;
  s.nchunks = (B + s.bchunk - 1) / s.bchunk;
  if (s.nchunks > 1) {
    HIP_CHECK(hipMemsetAsync((void*)gw, 0, (size_t)wn * sizeof(float),
                             S(stream)));
    if (gb)
      HIP_CHECK(hipMemsetAsync((void*)gb, 0, nb * sizeof(float),
                               S(stream)));
  }
  return s;
}

void conv2d_bwd(uintptr_t x, uintptr_t w, uintptr_t gy, uintptr_t gx,
                uintptr_t gw, uintptr_t gb, int B, int C, int H, int W,
                int K, int R, int S_, uintptr_t stream) {
  const int wn = K * C * R * S_;
  const Staging st = stage_for(wn);
  const int64_t n = (int64_t)B * C * H * W;
  hipLaunchKernelGGL(conv2d_bwd_x_kernel, dim3(grid_for(n, BLK)), dim3(BLK),
                     st.lds_bytes, S(stream), (const float*)gy,
                     (const float*)w, (float*)gx, B, C, H, W, K, R, S_,
                     st.staged);
  const BatchSplit sp = split_batch(B, wn, gw, gb, K, stream);
  hipLaunchKernelGGL(conv2d_bwd_w_kernel, dim3(sp.wtiles, sp.nchunks),
                     dim3(BLK), 0, S(stream), (const float*)x,
                     (const float*)gy, (float*)gw, (float*)gb, B, C, H, W,
                     K, R, S_, sp.bchunk);
}

void linear_fwd(uintptr_t x, uintptr_t w, uintptr_t bias, uintptr_t out,
                int B, int K, int N, bool fuse_relu, uintptr_t stream) {
  const Staging st = stage_for((int64_t)N * K);
  hipLaunchKernelGGL(linear_fwd_kernel,
                     dim3(grid_for((int64_t)B * N, BLK)), dim3(BLK),
                     st.lds_bytes, S(stream), (const float*)x,
                     (const float*)w, (const float*)bias, (float*)out, B, K,
                     N, fuse_relu ? 1 : 0, st.staged);
}

void linear_bwd(uintptr_t x, uintptr_t w, uintptr_t gy, uintptr_t out,
                uintptr_t gx, uintptr_t gw, uintptr_t gb, int B, int K,
                int N, uintptr_t stream) {
  const int wn = N * K;
  const Staging st = stage_for(wn);
  hipLaunchKernelGGL(linear_bwd_x_kernel,
                     dim3(grid_for((int64_t)B * K, BLK)), dim3(BLK),
                     st.lds_bytes, S(stream), (const float*)gy,
                     (const float*)out, (const float*)w, (float*)gx, B, K,
                     N, st.staged);
  const BatchSplit sp = split_batch(B, wn, gw, gb, N, stream);
  hipLaunchKernelGGL(linear_bwd_w_kernel, dim3(sp.wtiles, sp.nchunks),
                     dim3(BLK), 0, S(stream), (const float*)x,
                     (const float*)gy, (const float*)out, (float*)gw,
                     (float*)gb, B, K, N, sp.bchunk);
}

void log_softmax_fwd(uintptr_t x, uintptr_t out, int B, int N,
                     uintptr_t stream) {
  hipLaunchKernelGGL(log_softmax_fwd_kernel, dim3(grid_for(B, BLK)),
                     dim3(BLK), 0, S(stream), (const float*)x, (float*)out,
                     B, N);
}

void log_softmax_bwd(uintptr_t gy, uintptr_t out, uintptr_t gx, int B,
                     int N, uintptr_t stream) {
  hipLaunchKernelGGL(log_softmax_bwd_kernel, dim3(grid_for(B, BLK)),
                     dim3(BLK), 0, S(stream), (const float*)gy,
                     (const float*)out, (float*)gx, B, N);
}

void nll_loss_fwd(uintptr_t logp, uintptr_t target, uintptr_t loss, int B,
                  int N, uintptr_t stream) {
  HIP_CHECK(hipMemsetAsync((void*)loss, 0, sizeof(float), S(stream)));
  hipLaunchKernelGGL(nll_loss_fwd_kernel, dim3(grid_for(B, BLK)), dim3(BLK),
                     0, S(stream), (const float*)logp,
                     (const int64_t*)target, (float*)loss, B, N);
}

void nll_loss_bwd(uintptr_t target, uintptr_t gx, uintptr_t gloss, int B,
                  int N, uintptr_t stream) {
  hipLaunchKernelGGL(nll_loss_bwd_kernel, dim3(grid_for(B, BLK)), dim3(BLK),
                     0, S(stream), (const int64_t*)target, (float*)gx,
                     (const float*)gloss, B, N);
}

void log_softmax_nll_fwd(uintptr_t x, uintptr_t tgt, uintptr_t logp,
                         uintptr_t loss, int B, int N, uintptr_t stream) {
  HIP_CHECK(hipMemsetAsync((void*)loss, 0, sizeof(float), S(stream)));
  hipLaunchKernelGGL(log_softmax_nll_fwd_kernel, dim3(grid_for(B, BLK)),
                     dim3(BLK), 0, S(stream), (const float*)x,
                     (const int64_t*)tgt, (float*)logp, (float*)loss, B, N);
}

void log_softmax_nll_bwd(uintptr_t logp, uintptr_t tgt, uintptr_t gx,
                         uintptr_t gloss, int B, int N, uintptr_t stream) {
  hipLaunchKernelGGL(log_softmax_nll_bwd_kernel, dim3(grid_for(B, BLK)),
                     dim3(BLK), 0, S(stream), (const float*)logp,
                     (const int64_t*)tgt, (float*)gx, (const float*)gloss,
                     B, N);
}

void sgd_step(const std::vector<uintptr_t>& ps,
              const std::vector<uintptr_t>& gs,
              const std::vector<uintptr_t>& bufs,
              const std::vector<int64_t>& numels, double lr, double mu,
              bool zero_grad, uintptr_t stream, double weight_decay,
              bool nesterov) {
  if (weight_decay < 0)
    throw std::invalid_argument("sgd_step: weight_decay must be >= 0");
  if (nesterov) {
    if (mu == 0)
      throw std::invalid_argument("sgd_step: nesterov needs momentum");
    for (uintptr_t b : bufs)
      if (!b)
        throw std::invalid_argument(
            "sgd_step: nesterov needs a momentum buffer per tensor");
  }
  const bool wd = weight_decay != 0;
  auto kernel = nesterov ? (wd ? sgd_step_kernel<true, true>
                               : sgd_step_kernel<false, true>)
                         : (wd ? sgd_step_kernel<true, false>
                               : sgd_step_kernel<false, false>);
  size_t i = 0;
  while (i < ps.size()) {
    MtArgs a{};
    a.count = 0;
    a.total = 0;
    while (i < ps.size() && a.count < MT_MAX) {
      const int c = a.count;
      a.p[c] = (float*)ps[i];
      a.g[c] = (float*)gs[i];
      a.buf[c] = (float*)bufs[i];
      a.numel[c] = numels[i];
      a.offset[c] = a.total;
      a.total += numels[i];
      ++a.count;
      ++i;
    }
    hipLaunchKernelGGL(kernel, dim3(grid_for(a.total, BLK)), dim3(BLK), 0,
                       S(stream), a, (float)lr, (float)mu,
                       (float)weight_decay, zero_grad ? 1 : 0);
  }
}


// The reduction kernels move 16 bytes per access and divide the row
// stride by the vector width: a pointer or stride that breaks either
// would give wrong sums silently, so the launchers refuse it.
void require_aligned16(const char* op, const char* name, uintptr_t p) {
  if (p % 16 != 0)
    throw std::invalid_argument(std::string(op) + ": " + name +
                                " must be 16-byte aligned");
}

// The dtype argument of add_inplace and reduce_columns is the dist
// wrapper's _DTYPE code, NCCL's numbering: 7 is fp32 and 9 is bf16.
bool dtype_is_bf16(const char* op, int dtype) {
  if (dtype != 7 && dtype != 9)
    throw std::runtime_error(std::string(op) + ": unsupported dtype");
  return dtype == 9;
}

void add_inplace(uintptr_t dst, uintptr_t src, int64_t n, int dtype,
                 uintptr_t stream) {
  if (n < 0) throw std::invalid_argument("add_inplace: n must be >= 0");
  require_aligned16("add_inplace", "dst", dst);
  require_aligned16("add_inplace", "src", src);
  by_dtype(dtype_is_bf16("add_inplace", dtype), [&](auto* t) {
    using T = elem_t<decltype(t)>;
    constexpr int V = 16 / sizeof(T);
    hipLaunchKernelGGL(add_inplace_kernel<T>, dim3(grid_for(n, BLK, V)),
                       dim3(BLK), 0, S(stream), (T*)dst, (const T*)src, n);
  });
}

void reduce_columns(uintptr_t dst, uintptr_t src, int P, int64_t stride,
                    int64_t n, double scale, int dtype, uintptr_t stream) {
  if (n < 0 || P < 0)
    throw std::invalid_argument("reduce_columns: n and P must be >= 0");
  require_aligned16("reduce_columns", "dst", dst);
  by_dtype(dtype_is_bf16("reduce_columns", dtype), [&](auto* t) {
    using T = elem_t<decltype(t)>;
    constexpr int V = 16 / sizeof(T);
    if (P > 0) {  // P == 0 only scales dst and never reads src
      if (stride < 0 || stride % V != 0)
        throw std::invalid_argument(
            "reduce_columns: stride must be a multiple of " +
            std::to_string(V) + " elements, got " + std::to_string(stride));
      require_aligned16("reduce_columns", "src", src);
    }
    hipLaunchKernelGGL(reduce_columns_kernel<T>, dim3(grid_for(n, BLK, V)),
                       dim3(BLK), 0, S(stream), (T*)dst, (const T*)src, P,
                       stride, n, (float)scale);
  });
}

void scale_f32(uintptr_t dst, double s, int64_t n, uintptr_t stream) {
  if (n < 0) throw std::invalid_argument("scale_f32: n must be >= 0");
  require_aligned16("scale_f32", "dst", dst);
  hipLaunchKernelGGL(scale_f32_kernel, dim3(grid_for(n, BLK, 4)), dim3(BLK),
                     0, S(stream), (float*)dst, (float)s, n);
}

void copy_throttled(uintptr_t dst, uintptr_t src, int64_t n, int nblocks,
                    uintptr_t stream) {
  hipLaunchKernelGGL(copy_throttled_f32_kernel, dim3(nblocks), dim3(BLK),
                     0, S(stream), (float*)dst, (const float*)src, n);
}

}  // namespace

// K3-K6 (pool, ReLU, dropout and the bf16 cast, both dtypes) live in
// pointwise.hip, the fused whole-Net step in net_fused.hip, K16 (bf16 MFMA
// linear) in linear_bf16.hip, K17 (bf16 MFMA convolution) in
// conv_bf16.hip, K18 (batch normalization with fused add and ReLU) in
// batchnorm.hip, K19/K20 (general pooling) in pool.hip, K21 (cross-entropy
// for wide rows) in cross_entropy.hip
void register_pointwise(pybind11::module_& m);
void register_net_fused(pybind11::module_& m);
void register_linear_bf16(pybind11::module_& m);
void register_conv_bf16(pybind11::module_& m);
void register_batchnorm(pybind11::module_& m);
void register_pool(pybind11::module_& m);
void register_cross_entropy(pybind11::module_& m);

PYBIND11_MODULE(_kernels, m) {
  m.doc() = "CDNA4 HIP kernels for the dist_tuto_pth_amd training path";
  m.def("conv2d_fwd", &conv2d_fwd);
  m.def("conv2d_bwd", &conv2d_bwd);
  m.def("linear_fwd", &linear_fwd);
  m.def("linear_bwd", &linear_bwd);
  m.def("log_softmax_fwd", &log_softmax_fwd);
  m.def("log_softmax_bwd", &log_softmax_bwd);
  m.def("nll_loss_fwd", &nll_loss_fwd);
  m.def("nll_loss_bwd", &nll_loss_bwd);
  m.def("log_softmax_nll_fwd", &log_softmax_nll_fwd);
  m.def("log_softmax_nll_bwd", &log_softmax_nll_bwd);
  {
    namespace py = pybind11;
    // weight_decay and nesterov trail with defaults: the earlier
    // positional call keeps working
    m.def("sgd_step", &sgd_step, py::arg("ps"), py::arg("gs"),
          py::arg("bufs"), py::arg("numels"), py::arg("lr"), py::arg("mu"),
          py::arg("zero_grad"), py::arg("stream"),
          py::arg("weight_decay") = 0.0, py::arg("nesterov") = false);
  }
  m.def("add_inplace", &add_inplace);
  m.def("copy_throttled", &copy_throttled);
  m.def("reduce_columns", &reduce_columns);
  m.def("scale_f32", &scale_f32);
  register_pointwise(m);
  register_net_fused(m);
  register_linear_bf16(m);
  register_conv_bf16(m);
  register_batchnorm(m);
  register_pool(m);
  register_cross_entropy(m);
}
