// net_fused.hip — the fused whole-Net training step (gfx950/MI355X):
// everything that hard-codes Net's architecture.  Device code first
// (forward, data backward, weight-gradient partial / combine / fold,
// the single-launch cooperative step), then the host layer: one
// workspace layout, one chunk plan, one launcher per kernel group.
// Bindings are registered from kernels.hip's PYBIND11_MODULE through
// register_net_fused().

#include "common.h"

#include <hip/hip_cooperative_groups.h>

#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

namespace py = pybind11;

// ---- argument structs ----------------------------------------------------
// Plain aggregates of pointers and ints.  Who takes them, in one place:
//  - the host layer holds NetWs / GwPtrs and passes them, or their typed
//    members, to every launch;
//  - net_fused_fwdbwd_kernel and the two net_gw_partial_fold_kernel take
//    them by value;
//  - every other kernel and every device helper keeps a __restrict__
//    pointer list.  The helpers because the stashes mix floats with bytes
//    (idx1, m2, idx2, m3): a byte access may alias anything unless its
//    pointer is a __restrict__ PARAMETER, which neither a struct member
//    nor a local can be, and without it merged accesses split up.  The
//    kernels because each was slower, or spilled, with struct arguments
//    (profiles/net_fused_args.md has the figures).
//
// Per-batch workspace of the fused step (allocated by ops/fused.py).
// It crosses the binding as ONE pointer vector; NET_WS_FIELDS is the
// only definition of its order (exported as `ws_fields`).
static const char* const NET_WS_FIELDS[] = {
    "p1", "idx1", "m2", "p2", "idx2", "h1", "m3", "d3", "logp", "glog",
    "gh1", "ga2", "ga1", "part", "loss_part", "loss"};
constexpr int NET_WS_N = sizeof(NET_WS_FIELDS) / sizeof(NET_WS_FIELDS[0]);

struct NetWs {
  float* p1;         // [B,1440] pool1 out
  uint8_t* idx1;     // [B,1440] pool1 argmax (bit 2: relu cut it)
  uint8_t* m2;       // [B,20]   dropout2d keep mask
  float* p2;         // [B,320]  pool2 out
  uint8_t* idx2;     // [B,320]
  float* h1;         // [B,50]   fc1 out (post relu)
  uint8_t* m3;       // [B,50]   dropout keep mask
  float* d3;         // [B,50]   fc1 out after dropout
  float* logp;       // [B,10]
  float* glog;       // [B,10]   fc2 out grad
  float* gh1;        // [B,50]   fc1 pre-relu grad
  float* ga2;        // [B,1280] conv2 out grad
  float* ga1;        // [B,5760] conv1 out grad
  float* part;       // [GW_MAX_CH][GW_ROW] weight-gradient partials
  float* loss_part;  // [fwd grid] per-block loss partials
  float* loss;       // scalar
};
static_assert(sizeof(NetWs) == NET_WS_N * sizeof(void*),
              "NetWs has one pointer per NET_WS_FIELDS name, same order");

// The 8 per-parameter pointers (weights, gradients or momentum buffers;
// they may alias one flat buffer), slots in the order of the flat
// gradient layout OFF_W1 .. OFF_BF2.
struct GwPtrs { float* p[8]; };
enum { G_W1, G_B1, G_W2, G_B2, G_WF1, G_BF1, G_WF2, G_BF2 };

// A step's inputs (the fwd+bwd kernel's; its loss gradient is 1).
struct NetIn {
  const float* x;                  // [B,1,28,28]
  const int64_t* tgt;              // [B]
  const unsigned long long* seed;  // device dropout seed
  int B, training;
};

// fused step prologue: advance the dropout seed (when training) and
// zero the loss accumulator in ONE tiny launch instead of a bump
// kernel + a hipMemsetAsync fill kernel (each ~4.5 us of pure launch
// cost at the reference's batch sizes).
__global__ void step_prologue_kernel(unsigned long long* s, float* loss) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    if (s) *s += SEED_INC;
    *loss = 0.f;
  }
}

// ===========================================================================
// Fused whole-Net forward / backward (the launch-bound-regime lever).
//
// At the reference's batch sizes the per-op pipeline is bound by ~30
// kernel launches of ~5 us each, not by arithmetic (rocprof profile,
// profiles/).  These two kernels run the ENTIRE Net forward
// (train_dist.py:64-71: conv1 -> pool+relu -> conv2 -> dropout2d ->
// pool+relu -> fc1+relu -> dropout -> fc2 -> log_softmax -> NLL) and
// the entire data backward in ONE kernel each, one workgroup per batch
// element, activations staged through LDS; only the small per-batch
// weight-gradient reductions stay as separate (chunked) kernels.
// Architecture constants are Net's (SURVEY.md §2.1 'Net'): they are
// hard-coded, which is the point — this is the flagship model's fast
// path; the modular kernels of kernels.hip remain the general path.
// ===========================================================================
#define N_C1K 10        // conv1 out channels
#define N_C2K 20        // conv2 out channels
#define N_A1 (10*24*24) // conv1 out 5760
#define N_P1 (10*12*12) // pool1 out 1440
#define N_A2 (20*8*8)   // conv2 out 1280
#define N_P2 320        // pool2 out (= fc1 in)
#define N_H1 50         // fc1 out
#define N_CLS 10        // classes

// Stage stamps — DIAGNOSTIC BUILD ONLY (build.py --stage-stamps defines
// DTP_STAGE_STAMPS; the default build leaves it undefined and every
// STAGE_STAMP is empty).  Thread 0 of each workgroup stores the shader
// clock at the stage boundaries of net_fwd_sample / the data backward
// into a buffer of its own; benchmarks/stage_shares.py turns the
// differences into per-stage SHARES of a workgroup's time (the stamps
// perturb the kernels, so lengths are not to be quoted).
//   bwd: 0 entry, 1 w2 staged + sample start, 2 g_logits, 3 g_h1, 4 g_p2,
//        5 tile zeroed + scattered, 6 ga2 stashed (head done),
//        7 conv2-bwd_x partials done, 8 sample done
//   fwd: 9 entry, 10 x/w staged, 11 conv1+pool1, 12 conv2+pool2,
//        13 sibling hand-off done, 14 fc1, 15 fc2+softmax (sample done)
#ifdef DTP_STAGE_STAMPS
#define STAGE_NSTAMP 16
#define STAGE_NBLK 4096
__device__ unsigned long long g_stage_stamps[STAGE_NBLK * STAGE_NSTAMP];
#define STAGE_STAMP(i)                                                   \
  do {                                                                   \
    if (threadIdx.x == 0)                                                \
      g_stage_stamps[(blockIdx.x % STAGE_NBLK) * STAGE_NSTAMP + (i)] =   \
          (unsigned long long)clock64();                                 \
  } while (0)
#else
#define STAGE_STAMP(i) do {} while (0)
#endif

// partial-row access, parameterized on coherence: the in-launch fold
// variant stores partials sc1 (device-coherent, straight to the
// coherence point) and reads them back sc1 — ZERO fences, so the
// concurrently-running tile blocks keep their L1/L2 activation
// locality.  The first fold attempt used the plain-store + agent
// release/acquire recipe and measured 23-28% SLOWER end to end: one
// `buffer_wbl2` L2 writeback per block x 1744 blocks evicted the very
// activations the partial blocks re-read (ledger).  Partial traffic is
// ~1.8 MB/step, so the slower sc1 store path is immaterial.
template <bool SC1>
__device__ __forceinline__ void gw_st(float* p, float v) {
  if (SC1)
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else
    *p = v;
}
template <bool SC1>
__device__ __forceinline__ float gw_ld(const float* p) {
  if (SC1)
    return __hip_atomic_load(p, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
  return *p;
}

// One sample's full forward (conv1..log_softmax+NLL) by one 256-thread
// workgroup, activations staged through caller-provided LDS buffers.
// Returns -— on tid 0 only — the sample's log-prob at the target
// (callers accumulate the NLL loss); other lanes return 0.
// Shared by net_fused_fwdbwd_kernel, the single-launch net_step_kernel
// and the two 256-thread forward kernels below it, which net_fused_fwd
// runs only with DTP_FWD_TILED=0: its default is the re-blocked
// net_fused_fwd_tiled_kernel further down (same arguments, workspace,
// index bytes, dropout masks and hand-off; conv2's summation order
// differs).
// SPLIT mode (fused fwd at small B): TWO sibling workgroups per sample
// fill the otherwise half-idle chip (B=128 launches 128 blocks on 256
// CUs).  Both stage x/w1 and compute conv1+pool1 fully (duplicating
// the cheap stage costs less than a second exchange), each computes
// HALF of conv2's 20 output channels (and stages only its half of w2),
// sibling 1 publishes its p2 half with sc1 stores + a per-sample flag
// and exits; sibling 0 consumes it and runs fc1/fc2/softmax alone.
// If the sibling is not yet resident (co-residency is not contractual)
// sibling 0 falls back to computing the other half itself from its own
// LDS p1 — identical values, so the duplicate global stores are benign
// and the wait can never deadlock.
template <bool SPLIT = false>
__device__ __forceinline__ float net_fwd_sample(
    int b, int tid, int B, int training, uint64_t seed,
    int half, unsigned int* __restrict__ flag, unsigned int token,
    const float* __restrict__ x,
    const float* __restrict__ w1, const float* __restrict__ b1,
    const float* __restrict__ w2, const float* __restrict__ b2,
    const float* __restrict__ wf1, const float* __restrict__ bf1,
    const float* __restrict__ wf2, const float* __restrict__ bf2,
    const int64_t* __restrict__ tgt,
    float* __restrict__ p1_ws, uint8_t* __restrict__ idx1_ws,
    uint8_t* __restrict__ m2_ws, float* __restrict__ p2_ws,
    uint8_t* __restrict__ idx2_ws, float* __restrict__ h1_ws,
    uint8_t* __restrict__ m3_ws, float* __restrict__ d3_ws,
    float* __restrict__ logp_ws,
    // LDS carve (sizes: 784, 260, 1440, 5020, 320, 50, 10)
    float* xs, float* w1s, float* p1, float* w2s,
    float* p2, float* d3, float* logits) {
  float ret = 0.f;
  {
    STAGE_STAMP(9);
    // stage input + conv weights
    for (int i = tid; i < 784; i += 256) xs[i] = x[(int64_t)b * 784 + i];
    for (int i = tid; i < N_C1K * 25; i += 256) w1s[i] = w1[i];
    if (tid < N_C1K) w1s[N_C1K * 25 + tid] = b1[tid];
    {
      const int wlo = SPLIT ? half * (N_C2K / 2) * 250 : 0;
      const int whi = SPLIT ? wlo + (N_C2K / 2) * 250 : N_C2K * 250;
      for (int i = wlo + tid; i < whi; i += 256) w2s[i] = w2[i];
      const int klo = SPLIT ? half * (N_C2K / 2) : 0;
      const int khi = SPLIT ? klo + N_C2K / 2 : N_C2K;
      if (klo + tid < khi) w2s[N_C2K * 250 + klo + tid] = b2[klo + tid];
    }
    __syncthreads();
    STAGE_STAMP(10);

    // conv1 + pool1 + relu in ONE register-blocked stage: each thread
    // owns a 2x2 pooling window, computes its four conv outputs in
    // four independent accumulator chains (the kernel is LDS-latency
    // bound at ~1 wave/SIMD — profiles/), then pools in registers.
    // The 5760-float conv1 activation never touches LDS.
    for (int i = tid; i < N_P1; i += 256) {
      const int c = i / 144, ph = (i / 12) % 12, pw = i % 12;
      const float* wk = w1s + c * 25;
      const float* xp = xs + ph * 2 * 28 + pw * 2;
      const float bias = w1s[N_C1K * 25 + c];
      float q00 = bias, q01 = bias, q10 = bias, q11 = bias;
      #pragma unroll
      for (int r = 0; r < 5; ++r) {
        #pragma unroll
        for (int s = 0; s < 5; ++s) {
          const float w = wk[r * 5 + s];
          const float* xr = xp + r * 28 + s;
          q00 += xr[0] * w;
          q01 += xr[1] * w;
          q10 += xr[28] * w;
          q11 += xr[29] * w;
        }
      }
      int am = 0; float m = q00;
      if (q01 > m) { m = q01; am = 1; }
      if (q10 > m) { m = q10; am = 2; }
      if (q11 > m) { m = q11; am = 3; }
      const float o = m > 0.f ? m : 0.f;
      p1[i] = o;
      if (!SPLIT || half == 0) {
        p1_ws[(int64_t)b * N_P1 + i] = o;
        idx1_ws[(int64_t)b * N_P1 + i] =
            (uint8_t)(m > 0.f ? am : (am | 4));
      }
    }
    __syncthreads();
    STAGE_STAMP(11);

    // conv2 + dropout2d + pool2 + relu, same register-blocked shape:
    // one thread per pooled cell, four conv outputs in four chains,
    // channel dropout applied in registers before the max.
    const int c2lo = SPLIT ? half * (N_P2 / 2) : 0;
    const int c2hi = SPLIT ? c2lo + N_P2 / 2 : N_P2;
    for (int i = c2lo + tid; i < c2hi; i += 256) {
      const int k = i / 16, ph = (i / 4) % 4, pw = i % 4;
      const float bias = w2s[N_C2K * 250 + k];
      float q00 = bias, q01 = bias, q10 = bias, q11 = bias;
      #pragma unroll
      for (int c = 0; c < 10; ++c) {
        const float* pp = p1 + c * 144 + ph * 2 * 12 + pw * 2;
        const float* wc = w2s + (k * 10 + c) * 25;
        #pragma unroll
        for (int r = 0; r < 5; ++r) {
          #pragma unroll
          for (int s = 0; s < 5; ++s) {
            const float w = wc[r * 5 + s];
            const float* pr = pp + r * 12 + s;
            q00 += pr[0] * w;
            q01 += pr[1] * w;
            q10 += pr[12] * w;
            q11 += pr[13] * w;
          }
        }
      }
      if (training) {
        const uint32_t rr = mix32(seed, (uint64_t)b * N_C2K + k);
        const float dsc = (rr >= 0x80000000u) ? 2.f : 0.f;
        q00 *= dsc; q01 *= dsc; q10 *= dsc; q11 *= dsc;
      }
      int am = 0; float m = q00;
      if (q01 > m) { m = q01; am = 1; }
      if (q10 > m) { m = q10; am = 2; }
      if (q11 > m) { m = q11; am = 3; }
      const float o = m > 0.f ? m : 0.f;
      p2[i] = o;
      gw_st<SPLIT>(p2_ws + (int64_t)b * N_P2 + i, o);
      idx2_ws[(int64_t)b * N_P2 + i] = (uint8_t)(m > 0.f ? am : (am | 4));
    }
    if ((!SPLIT || half == 0) && training && tid < N_C2K) {
      const uint32_t rr = mix32(seed, (uint64_t)b * N_C2K + tid);
      m2_ws[(int64_t)b * N_C2K + tid] = rr >= 0x80000000u;
    }
    __syncthreads();
    STAGE_STAMP(12);
    if (SPLIT && half == 1) {
      // publish: p2 half is sc1-stored (at the coherence point once
      // vmcnt retires) — drain, then write this STEP's token.  A
      // token (not a 0/1 flag) makes stale publishes harmless: if a
      // fallback fired last step, this late write still never matches
      // a later step's expected token, so no reset is ever needed.
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (tid == 0)
        __hip_atomic_store(flag, token, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
      return 0.f;  // fc/softmax belong to sibling 0
    }
    if (SPLIT && half == 0) {
      // consume the sibling's half: bounded poll for THIS step's
      // token, then sc1 loads into our LDS p2.  On timeout compute
      // the half ourselves (fallback — co-residency is the norm but
      // not contractual).
      __shared__ unsigned s_got;
      if (tid == 0) {
        unsigned got = 0;
        for (int it = 0; it < 60000; ++it) {
          if (__hip_atomic_load(flag, __ATOMIC_RELAXED,
                                __HIP_MEMORY_SCOPE_AGENT) == token) {
            got = 1u;
            break;
          }
          __builtin_amdgcn_s_sleep(4);
        }
        if (got)  // consume: under hipGraph replay the token repeats,
                  // so the next replay must wait for a fresh publish
          __hip_atomic_store(flag, 0u, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
        s_got = got;
      }
      __syncthreads();
      if (s_got) {
        for (int i = N_P2 / 2 + tid; i < N_P2; i += 256)
          p2[i] = gw_ld<true>(p2_ws + (int64_t)b * N_P2 + i);
      } else {  // sibling never ran: do its channels from our own p1
        for (int i = N_P2 / 2 + tid; i < N_P2; i += 256) {
          const int k = i / 16, ph = (i / 4) % 4, pw = i % 4;
          float q00 = b2[k], q01 = q00, q10 = q00, q11 = q00;
          #pragma unroll
          for (int c = 0; c < 10; ++c) {
            const float* pp = p1 + c * 144 + ph * 2 * 12 + pw * 2;
            const float* wc = w2 + (k * 10 + c) * 25;  // global: our
            #pragma unroll                             // w2s half only
            for (int r = 0; r < 5; ++r) {
              #pragma unroll
              for (int s = 0; s < 5; ++s) {
                const float w = wc[r * 5 + s];
                const float* pr = pp + r * 12 + s;
                q00 += pr[0] * w;
                q01 += pr[1] * w;
                q10 += pr[12] * w;
                q11 += pr[13] * w;
              }
            }
          }
          if (training) {
            const uint32_t rr = mix32(seed, (uint64_t)b * N_C2K + k);
            const float dsc = (rr >= 0x80000000u) ? 2.f : 0.f;
            q00 *= dsc; q01 *= dsc; q10 *= dsc; q11 *= dsc;
          }
          float m = fmaxf(fmaxf(q00, q01), fmaxf(q10, q11));
          p2[i] = m > 0.f ? m : 0.f;
        }
      }
      __syncthreads();
    }

    STAGE_STAMP(13);
    // fc1 (320->50) + relu + dropout: 4 threads per output, shfl reduce
    if (tid < N_H1 * 4) {
      const int n = tid >> 2, q = tid & 3;
      const float* wr = wf1 + n * N_P2 + q * 80;
      const float* pr = p2 + q * 80;
      float e0 = 0.f, e1 = 0.f;
      #pragma unroll 4
      for (int k = 0; k < 80; k += 2) {
        e0 += pr[k] * wr[k];
        e1 += pr[k + 1] * wr[k + 1];
      }
      float acc = e0 + e1;
      acc += __shfl_down(acc, 1, 4);
      acc += __shfl_down(acc, 2, 4);
      if (q == 0) {
        float h = acc + bf1[n];
        h = h > 0.f ? h : 0.f;
        h1_ws[(int64_t)b * N_H1 + n] = h;
        float dd = h;
        uint8_t keep = 1;
        if (training) {
          const uint32_t rr = mix32(seed ^ 0x5bd1e995u,
                                    (uint64_t)b * N_H1 + n);
          keep = rr >= 0x80000000u;
          dd = keep ? h * 2.f : 0.f;
        }
        m3_ws[(int64_t)b * N_H1 + n] = keep;
        d3_ws[(int64_t)b * N_H1 + n] = dd;
        d3[n] = dd;
      }
    }
    __syncthreads();
    STAGE_STAMP(14);

    // fc2 (50->10)
    if (tid < N_CLS) {
      const float* wr = wf2 + tid * N_H1;
      float acc = bf2[tid];
      #pragma unroll 10
      for (int k = 0; k < N_H1; ++k) acc += d3[k] * wr[k];
      logits[tid] = acc;
    }
    __syncthreads();

    // log_softmax + NLL (one lane)
    if (tid == 0) {
      float m = logits[0];
      #pragma unroll
      for (int i = 1; i < N_CLS; ++i) m = fmaxf(m, logits[i]);
      float ssum = 0.f;
      #pragma unroll
      for (int i = 0; i < N_CLS; ++i) ssum += __expf(logits[i] - m);
      const float lse = m + __logf(ssum);
      float lp_t = 0.f;
      const int64_t t = tgt[b];
      #pragma unroll
      for (int i = 0; i < N_CLS; ++i) {
        const float lp = logits[i] - lse;
        logp_ws[(int64_t)b * N_CLS + i] = lp;
        if (i == (int)t) lp_t = lp;
      }
      ret = lp_t;
    }
    __syncthreads();
    STAGE_STAMP(15);
  }
  return ret;
}

__global__ void
__launch_bounds__(256)
net_fused_fwd_kernel(
    const float* __restrict__ x,      // [B,1,28,28]
    const float* __restrict__ w1, const float* __restrict__ b1,
    const float* __restrict__ w2, const float* __restrict__ b2,
    const float* __restrict__ wf1, const float* __restrict__ bf1,
    const float* __restrict__ wf2, const float* __restrict__ bf2,
    const int64_t* __restrict__ tgt,
    float* __restrict__ p1_ws,        // [B,1440]
    uint8_t* __restrict__ idx1_ws,    // [B,1440]
    uint8_t* __restrict__ m2_ws,      // [B,20]
    float* __restrict__ p2_ws,        // [B,320]
    uint8_t* __restrict__ idx2_ws,    // [B,320]
    float* __restrict__ h1_ws,        // [B,50]
    uint8_t* __restrict__ m3_ws,      // [B,50]
    float* __restrict__ d3_ws,        // [B,50]
    float* __restrict__ logp_ws,      // [B,10]
    float* __restrict__ loss,         // scalar (pre-zeroed) — legacy mode
    float* __restrict__ loss_part,    // [gridDim.x] or null: when set,
                                      // per-block partials (no atomics,
                                      // no pre-zeroing; the combine
                                      // kernel finalizes the loss)
    const unsigned long long* __restrict__ seed_p,
    int B, int training) {
  __shared__ __attribute__((aligned(16))) float xs[784];
  __shared__ float w1s[N_C1K * 25 + N_C1K];
  __shared__ float p1[N_P1];
  __shared__ float w2s[N_C2K * 10 * 25 + N_C2K];
  __shared__ float p2[N_P2];
  __shared__ float d3[N_H1];
  __shared__ float logits[N_CLS];
  const int tid = threadIdx.x;
  const uint64_t seed = seed_p[0];

  float lsum = 0.f;
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    const float lp_t = net_fwd_sample(
        b, tid, B, training, seed, 0, nullptr, 0u, x, w1, b1, w2, b2,
        wf1,
        bf1, wf2, bf2, tgt, p1_ws, idx1_ws, m2_ws, p2_ws, idx2_ws,
        h1_ws, m3_ws, d3_ws, logp_ws, xs, w1s, p1, w2s, p2, d3, logits);
    if (tid == 0) lsum += -lp_t / B;
  }
  if (tid == 0) {
    if (loss_part) loss_part[blockIdx.x] = lsum;
    else atomicAdd(loss, lsum);
  }
}

// Two sibling workgroups per sample (small-B fused fwd: B=128 alone
// leaves half the 256 CUs idle).  blockIdx.x = 2*b + half; sibling 1
// computes conv2 channels 10..19, publishes its p2 half (sc1 + flag)
// and exits; sibling 0 runs the rest.  Grid is exactly 2*B.
__global__ void
__launch_bounds__(256)
net_fused_fwd_split_kernel(
    const float* __restrict__ x,
    const float* __restrict__ w1, const float* __restrict__ b1,
    const float* __restrict__ w2, const float* __restrict__ b2,
    const float* __restrict__ wf1, const float* __restrict__ bf1,
    const float* __restrict__ wf2, const float* __restrict__ bf2,
    const int64_t* __restrict__ tgt,
    float* __restrict__ p1_ws, uint8_t* __restrict__ idx1_ws,
    uint8_t* __restrict__ m2_ws, float* __restrict__ p2_ws,
    uint8_t* __restrict__ idx2_ws, float* __restrict__ h1_ws,
    uint8_t* __restrict__ m3_ws, float* __restrict__ d3_ws,
    float* __restrict__ logp_ws, float* __restrict__ loss,
    float* __restrict__ loss_part,
    const unsigned long long* __restrict__ seed_p,
    int B, int training, unsigned int* __restrict__ flags,
    unsigned int token) {
  __shared__ __attribute__((aligned(16))) float xs[784];
  __shared__ float w1s[N_C1K * 25 + N_C1K];
  __shared__ float p1[N_P1];
  __shared__ float w2s[N_C2K * 10 * 25 + N_C2K];
  __shared__ float p2[N_P2];
  __shared__ float d3[N_H1];
  __shared__ float logits[N_CLS];
  const int tid = threadIdx.x;
  const uint64_t seed = seed_p[0];
  const int b = blockIdx.x >> 1, half = blockIdx.x & 1;
  const float lp_t = net_fwd_sample<true>(
      b, tid, B, training, seed, half, flags + b, token, x, w1, b1, w2,
      b2, wf1, bf1, wf2, bf2, tgt, p1_ws, idx1_ws, m2_ws, p2_ws,
      idx2_ws, h1_ws, m3_ws, d3_ws, logp_ws, xs, w1s, p1, w2s, p2, d3,
      logits);
  if (tid == 0) {
    const float lsum = half == 0 ? -lp_t / B : 0.f;
    if (loss_part) loss_part[blockIdx.x] = lsum;
    else if (half == 0) atomicAdd(loss, lsum);
  }
}

// The re-blocked forward (net_fused_fwd's default up to B=256, see
// fwd_tiled(); DTP_FWD_TILED=0 selects the two kernels above).  Same
// arguments, workspace and semantics, same sibling hand-off, 512
// threads, and the two conv stages
// in the shape of the tiled data backward: an item holds a 2x8 block of
// conv outputs in 16 accumulators and feeds 400 FMAs from 25 aligned
// 16-byte LDS reads (a 6-row x 12-column window as 18 float4, a filter
// padded to 28 floats as 7), where net_fwd_sample issues ~61 dword reads
// per 100 FMAs at one wave per SIMD.
//  - conv1 + pool1: item = (channel c, pooled row, group of 4 pooled
//    columns), 360 items in one round, c the fastest lane index.  The
//    accumulators start at the bias and run the taps in row-major order.
//  - conv2: item = (output channel k, pooled row, group g of CPG input
//    channels), 400 items either way: 10 k x 4 rows x 10 single channels
//    for a sibling, 20 k x 4 rows x 5 channel pairs unsplit.  Every
//    channel's 25 taps are summed from zero; a pair item adds its two
//    channel sums.  The partials go through LDS and one thread per pooled
//    cell adds them in ONE fixed order for both modes and the fallback,
//    ((((s01 + s23) + s45) + s67) + s89) + bias with s_ab = s_a + s_b,
//    then applies dropout, the 2x2 max, ReLU and the index byte.  So the
//    split and unsplit kernels, and the hand-off's fallback, give the
//    same bits.
//  - LDS strides (brute-force scan of the item -> lane maps against the
//    ds_read_b128 lane groups, profiles/convnet_step_history.md): filter
//    stride 28 with the (k, c) slot as the lane index, p1 plane stride
//    148 (37 quads, odd: ten channels land on ten bank quads; the
//    natural 144 puts all of them on the same four).
//  - fc1: 8 lanes per output on 400 lanes, ten float4 of wf1 per lane.
#define FT_NT 512    // threads
#define FT_WS 28     // staged filter stride
#define FT_PS 148    // p1 plane stride
#define FT_NITEM 400 // conv2 items
static_assert(FT_WS % 4 == 0 && FT_PS % 4 == 0 && FT_PS >= 144 &&
              FT_NITEM / 4 <= 128 && FT_NT == 4 * 128,
              "aligned float4 reads; a pooled row's items on 128 lanes");

// one input channel's 2x8 conv outputs: window rows 0..5 x 12 columns at
// xw (row r = float4 3r .. 3r+2 when RS4 == 3), filter at wk
template <int RS4>
__device__ __forceinline__ void ft_conv_2x8(const float4* xw,
                                            const float4* wk, float* q) {
  float xv[6][12], wv[28];
  #pragma unroll
  for (int r = 0; r < 6; ++r) {
    #pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float4 t = xw[r * RS4 + j];
      xv[r][4 * j] = t.x; xv[r][4 * j + 1] = t.y;
      xv[r][4 * j + 2] = t.z; xv[r][4 * j + 3] = t.w;
    }
  }
  #pragma unroll
  for (int j = 0; j < 7; ++j) {
    const float4 t = wk[j];
    wv[4 * j] = t.x; wv[4 * j + 1] = t.y;
    wv[4 * j + 2] = t.z; wv[4 * j + 3] = t.w;
  }
  #pragma unroll
  for (int r = 0; r < 5; ++r) {
    #pragma unroll
    for (int s = 0; s < 5; ++s) {
      #pragma unroll
      for (int a = 0; a < 2; ++a) {
        #pragma unroll
        for (int jj = 0; jj < 8; ++jj)
          q[a * 8 + jj] = fmaf(xv[a + r][jj + s], wv[r * 5 + s],
                               q[a * 8 + jj]);
      }
    }
  }
}

// 2x2 max (first maximum wins) + ReLU of one pooled cell; returns the
// index byte: window slot, bit 2 set when the ReLU is dead
__device__ __forceinline__ uint8_t ft_pool(float q00, float q01, float q10,
                                           float q11, float& o) {
  int am = 0; float m = q00;
  if (q01 > m) { m = q01; am = 1; }
  if (q10 > m) { m = q10; am = 2; }
  if (q11 > m) { m = q11; am = 3; }
  o = m > 0.f ? m : 0.f;
  return (uint8_t)(m > 0.f ? am : (am | 4));
}

template <bool SPLIT>
__global__ void
__launch_bounds__(FT_NT)
net_fused_fwd_tiled_kernel(
    const float* __restrict__ x,
    const float* __restrict__ w1, const float* __restrict__ b1,
    const float* __restrict__ w2, const float* __restrict__ b2,
    const float* __restrict__ wf1, const float* __restrict__ bf1,
    const float* __restrict__ wf2, const float* __restrict__ bf2,
    const int64_t* __restrict__ tgt,
    float* __restrict__ p1_ws, uint8_t* __restrict__ idx1_ws,
    uint8_t* __restrict__ m2_ws, float* __restrict__ p2_ws,
    uint8_t* __restrict__ idx2_ws, float* __restrict__ h1_ws,
    uint8_t* __restrict__ m3_ws, float* __restrict__ d3_ws,
    float* __restrict__ logp_ws, float* __restrict__ loss,
    float* __restrict__ loss_part,
    const unsigned long long* __restrict__ seed_p,
    int B, int training, unsigned int* __restrict__ flags,
    unsigned int token, int poll_bound) {
  constexpr int KL = SPLIT ? N_C2K / 2 : N_C2K;  // conv2 channels here
  constexpr int NG = SPLIT ? 10 : 5;             // input-channel groups
  constexpr int CPG = N_C1K / NG;                // channels per group
  static_assert(4 * KL * NG == FT_NITEM, "conv2 items");
  __shared__ __attribute__((aligned(16))) float xs[784];
  __shared__ __attribute__((aligned(16))) float w1p[N_C1K * FT_WS];
  __shared__ __attribute__((aligned(16))) float p1[N_C1K * FT_PS];
  __shared__ __attribute__((aligned(16))) float w2p[KL * N_C1K * FT_WS];
  __shared__ __attribute__((aligned(16))) float part[FT_NITEM * 16];
  __shared__ __attribute__((aligned(16))) float p2[N_P2];
  __shared__ float b1s[N_C1K];
  __shared__ float b2s[KL];
  __shared__ float d3[N_H1];
  __shared__ float logits[N_CLS];
  __shared__ unsigned s_got;
  const int tid = threadIdx.x;
  const uint64_t seed = seed_p[0];
  // split: blockIdx = 2b + half, the grid is exactly 2B
  const int half = SPLIT ? (blockIdx.x & 1) : 0;
  const int k0 = half * KL;

  STAGE_STAMP(9);
  // the weights are staged once per workgroup: w1 as [c][28], w2 as
  // [cc][k][g][28] for channel c = CPG*g + cc, so that consecutive
  // conv2 lanes (g fastest, then k) read consecutive 28-float slots
  for (int i = tid; i < N_C1K * 25; i += FT_NT) {
    const int c = i / 25, j = i - c * 25;
    w1p[c * FT_WS + j] = w1[i];
  }
  for (int i = tid; i < KL * N_C1K * 25; i += FT_NT) {
    const int kc = i / 25, j = i - kc * 25;
    const int kl = kc / N_C1K, c = kc - kl * N_C1K;
    const int slot = ((c % CPG) * KL + kl) * NG + c / CPG;
    w2p[slot * FT_WS + j] = w2[k0 * 250 + i];
  }
  if (tid < N_C1K) b1s[tid] = b1[tid];
  if (tid < KL) b2s[tid] = b2[k0 + tid];

  float lsum = 0.f;
  for (int b = SPLIT ? (int)(blockIdx.x >> 1) : (int)blockIdx.x; b < B;
       b += SPLIT ? B : (int)gridDim.x) {
    if (tid < 196)
      reinterpret_cast<float4*>(xs)[tid] =
          reinterpret_cast<const float4*>(x + (int64_t)b * 784)[tid];
    __syncthreads();
    STAGE_STAMP(10);

    // conv1 + pool1 + relu
    if (tid < 360) {
      const int c = tid % N_C1K, pg = tid / N_C1K;
      const int ph = pg / 3, g = pg - ph * 3;
      const float bias = b1s[c];
      float q[16];
      #pragma unroll
      for (int j = 0; j < 16; ++j) q[j] = bias;
      ft_conv_2x8<7>(
          reinterpret_cast<const float4*>(xs + ph * 2 * 28 + g * 8),
          reinterpret_cast<const float4*>(w1p + c * FT_WS), q);
      float o[4];
      uchar4 ib;
      ib.x = ft_pool(q[0], q[1], q[8], q[9], o[0]);
      ib.y = ft_pool(q[2], q[3], q[10], q[11], o[1]);
      ib.z = ft_pool(q[4], q[5], q[12], q[13], o[2]);
      ib.w = ft_pool(q[6], q[7], q[14], q[15], o[3]);
      const float4 o4 = make_float4(o[0], o[1], o[2], o[3]);
      const int cell = c * 144 + ph * 12 + g * 4;
      *reinterpret_cast<float4*>(p1 + c * FT_PS + ph * 12 + g * 4) = o4;
      if (!SPLIT || half == 0) {
        *reinterpret_cast<float4*>(p1_ws + (int64_t)b * N_P1 + cell) = o4;
        *reinterpret_cast<uchar4*>(idx1_ws + (int64_t)b * N_P1 + cell) = ib;
      }
    }
    __syncthreads();
    STAGE_STAMP(11);

    // conv2: per-group partial sums of a 2x8 output block
    // (a pooled row's 100 items sit on 128 lanes of their own: no wave
    // mixes two rows, which is what the bank scan assumes)
    if ((tid & 127) < NG * KL) {
      const int ph = tid >> 7, it = tid & 127;
      const int g = it % NG, kl = it / NG;
      const int item = ph * (NG * KL) + it;
      float q[16];
      #pragma unroll
      for (int cc = 0; cc < CPG; ++cc) {
        float t[16];
        #pragma unroll
        for (int j = 0; j < 16; ++j) t[j] = 0.f;
        ft_conv_2x8<3>(
            reinterpret_cast<const float4*>(p1 + (g * CPG + cc) * FT_PS +
                                            ph * 24),
            reinterpret_cast<const float4*>(
                w2p + ((cc * KL + kl) * NG + g) * FT_WS), t);
        #pragma unroll
        for (int j = 0; j < 16; ++j) q[j] = cc == 0 ? t[j] : q[j] + t[j];
      }
      // part[j][item]: consecutive lanes store consecutive float4
      #pragma unroll
      for (int j = 0; j < 4; ++j)
        reinterpret_cast<float4*>(part)[j * FT_NITEM + item] =
            make_float4(q[4 * j], q[4 * j + 1], q[4 * j + 2], q[4 * j + 3]);
    }
    __syncthreads();
    // fixed-order sum of the partials + bias, dropout2d, pool2 + relu
    if (tid < KL * 16) {
      const int kl = tid >> 4, ph = (tid >> 2) & 3, pw = tid & 3;
      const int k = k0 + kl;
      float v[4];
      #pragma unroll
      for (int a = 0; a < 2; ++a) {
        const float* pp = part + ((a * 2 + (pw >> 1)) * FT_NITEM +
                                  ph * (NG * KL) + kl * NG) * 4 + (pw & 1) * 2;
        float2 s = make_float2(0.f, 0.f);
        #pragma unroll
        for (int m = 0; m < 5; ++m) {
          // group g's partial is 4 floats on from group g - 1's
          float2 t = *reinterpret_cast<const float2*>(pp + m * (2 / CPG) * 4);
          if (CPG == 1) {  // single channels: pair them first
            const float2 u =
                *reinterpret_cast<const float2*>(pp + (m * 2 + 1) * 4);
            t.x += u.x; t.y += u.y;
          }
          s.x = m == 0 ? t.x : s.x + t.x;
          s.y = m == 0 ? t.y : s.y + t.y;
        }
        v[a * 2] = s.x + b2s[kl];
        v[a * 2 + 1] = s.y + b2s[kl];
      }
      if (training) {
        const uint32_t rr = mix32(seed, (uint64_t)b * N_C2K + k);
        const float dsc = (rr >= 0x80000000u) ? 2.f : 0.f;
        v[0] *= dsc; v[1] *= dsc; v[2] *= dsc; v[3] *= dsc;
      }
      float o;
      const uint8_t ib = ft_pool(v[0], v[1], v[2], v[3], o);
      const int i = k0 * 16 + tid;
      p2[i] = o;
      gw_st<SPLIT>(p2_ws + (int64_t)b * N_P2 + i, o);
      idx2_ws[(int64_t)b * N_P2 + i] = ib;
    }
    if ((!SPLIT || half == 0) && training && tid < N_C2K) {
      const uint32_t rr = mix32(seed, (uint64_t)b * N_C2K + tid);
      m2_ws[(int64_t)b * N_C2K + tid] = rr >= 0x80000000u;
    }
    __syncthreads();
    STAGE_STAMP(12);

    // the sibling hand-off: net_fwd_sample's protocol, unchanged
    if (SPLIT && half == 1) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (tid == 0) {
        __hip_atomic_store(flags + b, token, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        if (loss_part) loss_part[blockIdx.x] = 0.f;
      }
      return;  // fc/softmax belong to sibling 0
    }
    if (SPLIT) {
      if (tid == 0) {
        unsigned got = 0;
        for (int it = 0; it < poll_bound; ++it) {
          if (__hip_atomic_load(flags + b, __ATOMIC_RELAXED,
                                __HIP_MEMORY_SCOPE_AGENT) == token) {
            got = 1u;
            break;
          }
          __builtin_amdgcn_s_sleep(4);
        }
        if (got)  // consume, so a graph replay waits for a fresh publish
          __hip_atomic_store(flags + b, 0u, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
        s_got = got;
      }
      __syncthreads();
      if (s_got) {
        if (tid < N_P2 / 2)
          p2[N_P2 / 2 + tid] =
              gw_ld<true>(p2_ws + (int64_t)b * N_P2 + N_P2 / 2 + tid);
      } else if (tid < N_P2 / 2) {
        // the sibling is not resident yet: its channels from our own p1
        // and w2 in global memory, one pooled cell per thread (cold, so
        // at the old blocking), in the summation order of the items
        const int i = N_P2 / 2 + tid;
        const int k = i >> 4, ph = (i >> 2) & 3, pw = i & 3;
        float v[4];
        #pragma unroll 1
        for (int m = 0; m < 5; ++m) {
          float s[2][4];
          #pragma unroll
          for (int cc = 0; cc < 2; ++cc) {
            const int c = 2 * m + cc;
            const float* pp = p1 + c * FT_PS + ph * 24 + pw * 2;
            const float* wc = w2 + (k * N_C1K + c) * 25;
            float* t = s[cc];
            t[0] = t[1] = t[2] = t[3] = 0.f;
            #pragma unroll
            for (int r = 0; r < 5; ++r) {
              #pragma unroll
              for (int ss = 0; ss < 5; ++ss) {
                const float w = wc[r * 5 + ss];
                const float* pr = pp + r * 12 + ss;
                t[0] = fmaf(pr[0], w, t[0]);
                t[1] = fmaf(pr[1], w, t[1]);
                t[2] = fmaf(pr[12], w, t[2]);
                t[3] = fmaf(pr[13], w, t[3]);
              }
            }
          }
          #pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float sp = s[0][j] + s[1][j];
            v[j] = m == 0 ? sp : v[j] + sp;
          }
        }
        const float bias = b2[k];
        #pragma unroll
        for (int j = 0; j < 4; ++j) v[j] += bias;
        if (training) {
          const uint32_t rr = mix32(seed, (uint64_t)b * N_C2K + k);
          const float dsc = (rr >= 0x80000000u) ? 2.f : 0.f;
          v[0] *= dsc; v[1] *= dsc; v[2] *= dsc; v[3] *= dsc;
        }
        float o;
        ft_pool(v[0], v[1], v[2], v[3], o);
        p2[i] = o;
      }
      __syncthreads();
    }
    STAGE_STAMP(13);

    // fc1 (320->50) + relu + dropout: 8 lanes per output, shfl reduce.
    // The pointer is opaque per sample so that the ten wf1 loads are not
    // hoisted out of the sample loop (registers).
    if (tid < N_H1 * 8) {
      const int n = tid >> 3, q8 = tid & 7;
      const float* wf1_b = wf1;
      asm volatile("" : "+s"(wf1_b));
      const float4* wr =
          reinterpret_cast<const float4*>(wf1_b + n * N_P2 + q8 * 40);
      const float4* pr = reinterpret_cast<const float4*>(p2 + q8 * 40);
      float4 wv[10];
      #pragma unroll
      for (int j = 0; j < 10; ++j) wv[j] = wr[j];
      float e0 = 0.f, e1 = 0.f, e2 = 0.f, e3 = 0.f;
      #pragma unroll
      for (int j = 0; j < 10; ++j) {
        const float4 pv = pr[j];
        e0 = fmaf(pv.x, wv[j].x, e0);
        e1 = fmaf(pv.y, wv[j].y, e1);
        e2 = fmaf(pv.z, wv[j].z, e2);
        e3 = fmaf(pv.w, wv[j].w, e3);
      }
      float acc = (e0 + e1) + (e2 + e3);
      acc += __shfl_down(acc, 1, 8);
      acc += __shfl_down(acc, 2, 8);
      acc += __shfl_down(acc, 4, 8);
      if (q8 == 0) {
        float h = acc + bf1[n];
        h = h > 0.f ? h : 0.f;
        h1_ws[(int64_t)b * N_H1 + n] = h;
        float dd = h;
        uint8_t keep = 1;
        if (training) {
          const uint32_t rr = mix32(seed ^ 0x5bd1e995u,
                                    (uint64_t)b * N_H1 + n);
          keep = rr >= 0x80000000u;
          dd = keep ? h * 2.f : 0.f;
        }
        m3_ws[(int64_t)b * N_H1 + n] = keep;
        d3_ws[(int64_t)b * N_H1 + n] = dd;
        d3[n] = dd;
      }
    }
    __syncthreads();
    STAGE_STAMP(14);

    // fc2 (50->10), then log_softmax + NLL on one lane, as net_fwd_sample
    if (tid < N_CLS) {
      const float* wr = wf2 + tid * N_H1;
      float acc = bf2[tid];
      #pragma unroll 10
      for (int kk = 0; kk < N_H1; ++kk) acc += d3[kk] * wr[kk];
      logits[tid] = acc;
    }
    __syncthreads();
    if (tid == 0) {
      float m = logits[0];
      #pragma unroll
      for (int i = 1; i < N_CLS; ++i) m = fmaxf(m, logits[i]);
      float ssum = 0.f;
      #pragma unroll
      for (int i = 0; i < N_CLS; ++i) ssum += __expf(logits[i] - m);
      const float lse = m + __logf(ssum);
      float lp_t = 0.f;
      const int64_t t = tgt[b];
      #pragma unroll
      for (int i = 0; i < N_CLS; ++i) {
        const float lp = logits[i] - lse;
        logp_ws[(int64_t)b * N_CLS + i] = lp;
        if (i == (int)t) lp_t = lp;
      }
      lsum += -lp_t / B;
    }
    __syncthreads();
    STAGE_STAMP(15);
  }
  if (tid == 0) {
    if (loss_part) loss_part[blockIdx.x] = lsum;
    else atomicAdd(loss, lsum);
  }
}

// The head of one sample's data backward: loss grad -> the zero-padded
// conv2-out grad tile gd2p[k][16][RS] (plane stride PS; entry
// (k, oh+4, ow+4) holds the conv2-out grad at [k][oh][ow]) by an
// NT-thread workgroup.  Every sibling of a sample recomputes it (~35k
// FMA); sibling 0 also writes glog / gh1 / ga2 for the weight-gradient
// pass.  Ends on a barrier: the tile is complete for all threads.
template <int NT, int RS, int PS>
__device__ __forceinline__ void net_bwd_head(
    int b, int half, int tid, int training, float sc,
    const float* __restrict__ wf1, const float* __restrict__ wf2,
    const int64_t* __restrict__ tgt,
    const uint8_t* __restrict__ m2_ws,
    const uint8_t* __restrict__ idx2_ws,
    const float* __restrict__ h1_ws,
    const uint8_t* __restrict__ m3_ws,
    const float* __restrict__ logp_ws,
    float* __restrict__ glog_ws, float* __restrict__ gh1_ws,
    float* __restrict__ ga2_ws,
    // LDS carve (sizes: 10, 50, 50, 320, 20 * PS)
    float* glg, float* gd3, float* gh1, float* gp2, float* gd2p) {
  {
    // g_logits = (exp(logp) - onehot) * gl / B
    __syncthreads();
    STAGE_STAMP(1);
    if (tid < N_CLS) {
      const float lp = logp_ws[(int64_t)b * N_CLS + tid];
      const float g = (__expf(lp) -
                       (tid == (int)tgt[b] ? 1.f : 0.f)) * sc;
      glg[tid] = g;
      if (half == 0)
        glog_ws[(int64_t)b * N_CLS + tid] = g;
    }
    __syncthreads();
    STAGE_STAMP(2);

    // g_d3 = wf2^T g_logits ; through dropout + relu -> g_h1pre
    if (tid < N_H1) {
      float acc = 0.f;
      #pragma unroll
      for (int n = 0; n < N_CLS; ++n)
        acc += wf2[n * N_H1 + tid] * glg[n];
      gd3[tid] = acc;
      float g = acc;
      if (training) {
        g = m3_ws[(int64_t)b * N_H1 + tid] ? g * 2.f : 0.f;
      }
      if (h1_ws[(int64_t)b * N_H1 + tid] <= 0.f) g = 0.f;
      gh1[tid] = g;
      if (half == 0)
        gh1_ws[(int64_t)b * N_H1 + tid] = g;
    }
    __syncthreads();
    STAGE_STAMP(3);

    // g_p2 = wf1^T g_h1pre  (320 outputs x 50), four accumulator
    // chains over the reduction dim (wf1 rows are coalesced global
    // reads; the single 50-deep load+FMA chain was latency-bound)
    for (int i = tid; i < N_P2; i += NT) {
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
      #pragma unroll
      for (int n = 0; n < 48; n += 4) {
        a0 += wf1[n * N_P2 + i] * gh1[n];
        a1 += wf1[(n + 1) * N_P2 + i] * gh1[n + 1];
        a2 += wf1[(n + 2) * N_P2 + i] * gh1[n + 2];
        a3 += wf1[(n + 3) * N_P2 + i] * gh1[n + 3];
      }
      a0 += wf1[48 * N_P2 + i] * gh1[48];
      a1 += wf1[49 * N_P2 + i] * gh1[49];
      gp2[i] = (a0 + a1) + (a2 + a3);
    }
    __syncthreads();
    STAGE_STAMP(4);

    // pool2 bwd + dropout2d bwd -> g_a2, scattered STRAIGHT into the
    // padded gd2p tile with dropout applied (r2: the old path staged
    // through a dense gd2 buffer — zero + scatter + full re-read, an
    // extra 2.5k LDS ops per sample for nothing; gd2 is gone)
    for (int i = tid; i < N_C2K * PS; i += NT) gd2p[i] = 0.f;
    __syncthreads();
    for (int i = tid; i < N_P2; i += NT) {
      const int c = i / 16, oh = (i / 4) % 4, ow = i % 4;
      const uint8_t v = idx2_ws[(int64_t)b * N_P2 + i];
      if (!(v & 4)) {
        const int am = v & 3;
        const int fr = oh * 2 + (am >> 1), fc = ow * 2 + (am & 1);
        float g = gp2[i];
        if (training)
          g = m2_ws[(int64_t)b * N_C2K + c] ? g * 2.f : 0.f;
        gd2p[c * PS + (fr + 4) * RS + (fc + 4)] = g;
      }
    }
    __syncthreads();
    STAGE_STAMP(5);
    if (half == 0) {  // stash the dense conv2-out grad for the gw pass
      for (int i = tid; i < N_A2; i += NT) {
        const int k = i / 64, oh = (i / 8) % 8, ow = i % 8;
        ga2_ws[(int64_t)b * N_A2 + i] =
            gd2p[k * PS + (oh + 4) * RS + (ow + 4)];
      }
    }
    __syncthreads();
    STAGE_STAMP(6);
  }
}

// One (sample, sibling-half)'s data backward: loss grad -> g_a1 (conv1
// output grad).  `split` sibling workgroups cooperate on each sample:
// the cheap early stages (g_logits .. gd2p staging, ~35k FMA) are
// recomputed by every sibling, the hot conv2-bwd_x stage (720k FMA) is
// partitioned by pooled position.  w2s must be pre-staged with conv2's
// weights (5000 floats) by the caller.  Shared by net_fused_bwd_kernel
// and the single-launch net_step_kernel.
__device__ __forceinline__ void net_bwd_sample(
    int b, int half, int split, int tid, int B, int training, float sc,
    const float* __restrict__ wf1, const float* __restrict__ wf2,
    const int64_t* __restrict__ tgt,
    const uint8_t* __restrict__ idx1_ws,
    const uint8_t* __restrict__ m2_ws,
    const uint8_t* __restrict__ idx2_ws,
    const float* __restrict__ h1_ws,
    const uint8_t* __restrict__ m3_ws,
    const float* __restrict__ logp_ws,
    float* __restrict__ glog_ws, float* __restrict__ gh1_ws,
    float* __restrict__ ga2_ws, float* __restrict__ ga1_ws,
    // LDS carve (sizes: 5000, 10, 50, 50, 320, 6080)
    const float* w2s, float* glg, float* gd3, float* gh1, float* gp2,
    float* gd2p) {
  net_bwd_head<256, 19, 304>(b, half, tid, training, sc, wf1, wf2, tgt,
                             m2_ws, idx2_ws, h1_ws, m3_ws, logp_ws, glog_ws,
                             gh1_ws, ga2_ws, glg, gd3, gh1, gp2, gd2p);
  {
    // conv2 bwd_x through the padded tile + pool1 bwd, register-blocked
    // 4-wide: each thread owns FOUR horizontally-adjacent pooled
    // positions (one accumulator chain each); a (k, r) row contributes
    // 8 consecutive gd2p values shared by all four outputs, cutting
    // LDS reads ~2.5x vs one-output-per-thread (the kernel is
    // LDS-latency-bound at this occupancy — profiles/).  Each pooled
    // position owns its 2x2 ga1 window exclusively, so all four slots
    // are written with no zeroing pass.  Partitioned across the
    // `split` sibling workgroups (360 strips divisible by 1/2/4/8).
    const int seg = (N_P1 / 4) / split;
    const int t_end = (half + 1) * seg;
    for (int t = half * seg + tid; t < t_end; t += 256) {
      const int c = t / 36, rem = t % 36;
      const int h = rem / 3, wc0 = (rem % 3) * 4;
      float q0 = 0.f, q1 = 0.f, q2 = 0.f, q3 = 0.f;
      for (int k = 0; k < N_C2K; ++k) {
        const float* gk = gd2p + k * 304;
        const float* wk = w2s + (k * 10 + c) * 25;
        #pragma unroll
        for (int r = 0; r < 5; ++r) {
          const float* row = gk + (h - r + 4) * 19 + wc0;
          const float w0 = wk[r * 5 + 0], w1 = wk[r * 5 + 1];
          const float w2v = wk[r * 5 + 2], w3 = wk[r * 5 + 3];
          const float w4 = wk[r * 5 + 4];
          const float e0 = row[0], e1 = row[1], e2 = row[2];
          const float e3 = row[3], e4 = row[4], e5 = row[5];
          const float e6 = row[6], e7 = row[7];
          q0 += e4 * w0 + e3 * w1 + e2 * w2v + e1 * w3 + e0 * w4;
          q1 += e5 * w0 + e4 * w1 + e3 * w2v + e2 * w3 + e1 * w4;
          q2 += e6 * w0 + e5 * w1 + e4 * w2v + e3 * w3 + e2 * w4;
          q3 += e7 * w0 + e6 * w1 + e5 * w2v + e4 * w3 + e3 * w4;
        }
      }
      const float qq[4] = {q0, q1, q2, q3};
      const int64_t ib = (int64_t)b * N_P1 + c * 144 + h * 12 + wc0;
      float* gp_base = ga1_ws + (int64_t)b * N_A1 + c * 576 +
                       h * 2 * 24 + wc0 * 2;
      #pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint8_t v = idx1_ws[ib + j];
        const int am = v & 3;
        const float g = (v & 4) ? 0.f : qq[j];
        float* gp = gp_base + j * 2;
        gp[0] = am == 0 ? g : 0.f;
        gp[1] = am == 1 ? g : 0.f;
        gp[24] = am == 2 ? g : 0.f;
        gp[25] = am == 3 ? g : 0.f;
      }
    }
    __syncthreads();
    STAGE_STAMP(8);
  }
}

// Fused data-gradient backward: from loss grad to g_a1 (conv1 output
// grad) in one kernel; weight gradients are reduced afterwards by the
// chunked partial/combine kernels over the stashes.
__global__ void
__launch_bounds__(256)
net_fused_bwd_kernel(
    // pointer by pointer, not NetWs by value: the struct form measured
    // slower in the tiled kernel (profiles/net_fused_args.md), and the
    // host picks between the two through one function pointer
    const float* __restrict__ w2, const float* __restrict__ wf1,
    const float* __restrict__ wf2,
    const int64_t* __restrict__ tgt,
    const float* __restrict__ gl,      // dLoss (device scalar)
    const uint8_t* __restrict__ idx1_ws,
    const uint8_t* __restrict__ m2_ws,
    const uint8_t* __restrict__ idx2_ws,
    const float* __restrict__ h1_ws,
    const uint8_t* __restrict__ m3_ws,
    const float* __restrict__ logp_ws,
    float* __restrict__ glog_ws,       // [B,10]  (fc2 out grad)
    float* __restrict__ gh1_ws,        // [B,50]  (fc1 pre-relu grad)
    float* __restrict__ ga2_ws,        // [B,1280] (conv2 out grad)
    float* __restrict__ ga1_ws,        // [B,5760] (conv1 out grad)
    int B, int training, int split) {
  __shared__ __attribute__((aligned(16))) float w2s[N_C2K * 250];
  __shared__ float glg[N_CLS];
  __shared__ float gd3[N_H1];
  __shared__ float gh1[N_H1];
  __shared__ float gp2[N_P2];
  // zero-padded conv2-out grad [k][16][19]: entry (k,oh+4,ow+4) holds
  // the conv2-out grad at [k][oh][ow]; the pad makes the transposed-
  // conv window reads branch-free so the 500-FMA loop unrolls with
  // ILP.  Row stride 19 (not 16): PMC measured 59.8% LDSBankConflict
  // at B=4096 from the power-of-2 stride (profiles/pmc_r2.md); over
  // the loop's (h, wc0) lane pattern a brute-force scan shows stride
  // 19 is conflict-FREE on 64 banks (17 still left 3-way clusters).
  __shared__ float gd2p[N_C2K * 304];
  const int tid = threadIdx.x;

  STAGE_STAMP(0);
  for (int i = tid; i < N_C2K * 250; i += 256) w2s[i] = w2[i];
  const float sc = gl[0] / B;

  for (int bb = blockIdx.x; bb < B * split; bb += gridDim.x) {
    net_bwd_sample(bb / split, bb % split, split, tid, B, training, sc,
                   wf1, wf2, tgt, idx1_ws, m2_ws, idx2_ws, h1_ws, m3_ws,
                   logp_ws, glog_ws, gh1_ws, ga2_ws, ga1_ws,
                   w2s, glg, gd3, gh1, gp2, gd2p);
  }
}

// The data backward with the conv2-bwd_x loop re-blocked for 16-byte LDS
// reads and full SIMDs (512 threads = 2 waves per SIMD).  Same head as
// net_fused_bwd_kernel; the hot loop differs:
//  - a work item is a 2-row x 4-wide tile of pooled positions (pos =
//    hp*3 + wq, 18 per channel) of one input channel c, over ONE group
//    of 4 of conv2's 20 output channels k.  Per k it reads 6 rows x 8
//    floats of the padded tile and the 25-float filter — 12 + 7
//    ds_read_b128 — and feeds 200 FMAs; the five k-group partials of a
//    tile are summed through LDS in fixed order (no atomics:
//    deterministic, and the value does not depend on `split`).
//  - tile row stride 20, plane stride 332: a row segment is two aligned
//    float4.  Brute-force scan over the item -> lane map below against
//    the ds_read_b128 lane groups (4 x 16 lanes, 16 bank quads): with
//    the channel as the fastest lane index, (20, 332) is conflict-free
//    (4 LDS cycles per read) for 90-tile rounds of 5 or 10 channels;
//    plane strides 320/324/328 cost 4.25-4.75, row stride 16 5.0-6.0,
//    and a position-fastest lane order 7.75 or more at any stride.
//  - w2 is staged as [k][c_local][28]: each (k, c) filter 16-byte
//    aligned, and only this sibling's input channels (half of w2 at
//    split >= 2).  Lanes of equal c read one address (broadcast).
//  - siblings partition (channel half) x (position range): split = 1
//    owns everything, 2 a channel half, 4 and 8 cut each half's 18
//    positions into 2 and 4 ranges.  A round is <= 90 tiles x 5 k-groups
//    = 450 of 512 lanes (88%).
#define BT_NT 512   // threads
#define BT_RS 20    // tile row stride (floats)
#define BT_PS 332   // tile plane stride
#define BT_WS 28    // staged filter stride
#define BT_KG 5     // k groups (of N_C2K / BT_KG = 4 channels)
#define BT_ROUND 90 // tiles per round: BT_ROUND * BT_KG <= BT_NT
static_assert(BT_ROUND * BT_KG <= BT_NT, "one item per thread per round");
static_assert(BT_RS % 4 == 0 && BT_PS % 4 == 0 && BT_WS % 4 == 0 &&
              BT_PS >= 16 * BT_RS && BT_WS >= 25, "aligned float4 reads");

__global__ void
__launch_bounds__(BT_NT)
net_fused_bwd_tiled_kernel(
    const float* __restrict__ w2, const float* __restrict__ wf1,
    const float* __restrict__ wf2,
    const int64_t* __restrict__ tgt,
    const float* __restrict__ gl,      // dLoss (device scalar)
    const uint8_t* __restrict__ idx1_ws,
    const uint8_t* __restrict__ m2_ws,
    const uint8_t* __restrict__ idx2_ws,
    const float* __restrict__ h1_ws,
    const uint8_t* __restrict__ m3_ws,
    const float* __restrict__ logp_ws,
    float* __restrict__ glog_ws, float* __restrict__ gh1_ws,
    float* __restrict__ ga2_ws, float* __restrict__ ga1_ws,
    int B, int training, int split) {
  __shared__ __attribute__((aligned(16))) float w2p[N_C2K * N_C1K * BT_WS];
  __shared__ __attribute__((aligned(16))) float gd2p[N_C2K * BT_PS];
  __shared__ __attribute__((aligned(16))) float part[BT_ROUND * BT_KG * 8];
  __shared__ float glg[N_CLS];
  __shared__ float gd3[N_H1];
  __shared__ float gh1[N_H1];
  __shared__ float gp2[N_P2];
  const int tid = threadIdx.x;

  // the grid is B * split or a multiple of 8 (host), so a workgroup
  // keeps one sibling index over its grid-stride loop
  const int half = blockIdx.x % split;
  const int cgs = split >= 2 ? 2 : 1, prs = split / cgs;
  const int nc = N_C1K / cgs, c0 = (half / prs) * nc;
  const int p0 = 18 * (half % prs) / prs;
  const int p1 = 18 * (half % prs + 1) / prs;
  const int ppr = BT_ROUND / nc;  // positions per round

  STAGE_STAMP(0);
  for (int i = tid; i < N_C2K * nc * 25; i += BT_NT) {
    const int kc = i / 25, j = i - kc * 25;
    const int k = kc / nc, cl = kc - k * nc;
    w2p[kc * BT_WS + j] = w2[(k * N_C1K + c0 + cl) * 25 + j];
  }
  const float sc = gl[0] / B;

  for (int bb = blockIdx.x; bb < B * split; bb += gridDim.x) {
    const int b = bb / split;
    // (its leading barrier also orders the w2p staging and the previous
    // sample's last tile reads)
    // opaque per sample: with one g_p2 output per lane the 50 wf1
    // loads are loop-invariant, and hoisted out of this loop they
    // spilled 105 registers to scratch
    const float* wf1_b = wf1;
    asm volatile("" : "+s"(wf1_b));
    net_bwd_head<BT_NT, BT_RS, BT_PS>(
        b, half, tid, training, sc, wf1_b, wf2, tgt, m2_ws, idx2_ws, h1_ws,
        m3_ws, logp_ws, glog_ws, gh1_ws, ga2_ws, glg, gd3, gh1, gp2, gd2p);

    for (int pb = p0; pb < p1; pb += ppr) {
      const int nt = min(ppr, p1 - pb) * nc;  // tiles this round
      if (tid < nt * BT_KG) {
        const int kg = tid / nt, tl = tid - kg * nt;
        const int pl = tl / nc, cl = tl - pl * nc;
        const int pos = pb + pl, hp = pos / 3, wc0 = (pos % 3) * 4;
        // rows 2hp .. 2hp+5 of the padded tile cover both output rows'
        // five filter rows; columns wc0 .. wc0+7 all four outputs' taps
        const float4* gk = reinterpret_cast<const float4*>(
            gd2p + kg * (N_C2K / BT_KG) * BT_PS + 2 * hp * BT_RS + wc0);
        const float4* wk = reinterpret_cast<const float4*>(
            w2p + (kg * (N_C2K / BT_KG) * nc + cl) * BT_WS);
        const int wstep = nc * (BT_WS / 4);
        float q[8];
        #pragma unroll
        for (int j = 0; j < 8; ++j) q[j] = 0.f;
        // two register sets in ping-pong: the other set's reads (next k)
        // are issued ahead of this set's arithmetic.  The pair loop is
        // NOT unrolled: fully unrolled, the scheduler hoisted all four
        // k's reads (4 x 76 registers) and spilled to scratch.
        float4 ea[12], wa[7], eb[12], wb[7];
        auto load = [&](float4* e, float4* w, int kk) {
          const float4* gn = gk + kk * (BT_PS / 4);
          const float4* wn = wk + kk * wstep;
          #pragma unroll
          for (int j = 0; j < 6; ++j) {
            e[2 * j] = gn[j * (BT_RS / 4)];
            e[2 * j + 1] = gn[j * (BT_RS / 4) + 1];
          }
          #pragma unroll
          for (int j = 0; j < 7; ++j) w[j] = wn[j];
        };
        // out(h, w) += g[k][h - r][w - s] * w2[k][c][r][s]; tile entry
        // (oh + 4, ow + 4) -> local row a - r + 4, local col jj + 4 - s
        auto fma200 = [&](const float4* e, const float4* w) {
          float ev[6][8], wv[28];
          #pragma unroll
          for (int j = 0; j < 12; ++j) {
            ev[j >> 1][(j & 1) * 4 + 0] = e[j].x;
            ev[j >> 1][(j & 1) * 4 + 1] = e[j].y;
            ev[j >> 1][(j & 1) * 4 + 2] = e[j].z;
            ev[j >> 1][(j & 1) * 4 + 3] = e[j].w;
          }
          #pragma unroll
          for (int j = 0; j < 7; ++j) {
            wv[4 * j] = w[j].x; wv[4 * j + 1] = w[j].y;
            wv[4 * j + 2] = w[j].z; wv[4 * j + 3] = w[j].w;
          }
          #pragma unroll
          for (int r = 0; r < 5; ++r) {
            #pragma unroll
            for (int s = 0; s < 5; ++s) {
              #pragma unroll
              for (int a = 0; a < 2; ++a) {
                #pragma unroll
                for (int jj = 0; jj < 4; ++jj)
                  q[a * 4 + jj] = fmaf(ev[a - r + 4][jj + 4 - s],
                                       wv[r * 5 + s], q[a * 4 + jj]);
              }
            }
          }
        };
        static_assert((N_C2K / BT_KG) % 2 == 0, "k pairs");
        load(ea, wa, 0);
        #pragma unroll 1
        for (int kk = 0; kk < N_C2K / BT_KG; kk += 2) {
          load(eb, wb, kk + 1);
          fma200(ea, wa);
          // (the last pair re-reads its own second k: in bounds, unused)
          load(ea, wa, min(kk + 2, N_C2K / BT_KG - 1));
          fma200(eb, wb);
        }
        float4* pp = reinterpret_cast<float4*>(part + tid * 8);
        pp[0] = make_float4(q[0], q[1], q[2], q[3]);
        pp[1] = make_float4(q[4], q[5], q[6], q[7]);
      }
      __syncthreads();
      STAGE_STAMP(7);
      // fixed-order sum of the k-group partials, then pool1 bwd: each
      // pooled position owns its 2x2 ga1 window, all four slots written
      for (int o = tid; o < nt * 8; o += BT_NT) {
        const int tl = o >> 3, j = o & 7;
        float g = part[o];
        #pragma unroll
        for (int kg = 1; kg < BT_KG; ++kg) g += part[kg * nt * 8 + o];
        const int pl = tl / nc, c = c0 + tl - pl * nc;
        const int pos = pb + pl;
        const int h = (pos / 3) * 2 + (j >> 2), wc = (pos % 3) * 4 + (j & 3);
        const uint8_t v = idx1_ws[(int64_t)b * N_P1 + c * 144 + h * 12 + wc];
        const int am = v & 3;
        if (v & 4) g = 0.f;
        float* gp = ga1_ws + (int64_t)b * N_A1 + c * 576 + h * 2 * 24 +
                    wc * 2;
        *reinterpret_cast<float2*>(gp) =
            make_float2(am == 0 ? g : 0.f, am == 1 ? g : 0.f);
        *reinterpret_cast<float2*>(gp + 24) =
            make_float2(am == 2 ? g : 0.f, am == 3 ? g : 0.f);
      }
      __syncthreads();
    }
    STAGE_STAMP(8);
  }
}

// Combined forward + data-backward in ONE kernel (round-2 experiment,
// VERDICT r1 #9).  In the training loop the loss gradient is the
// constant 1, so sample b's data backward depends ONLY on sample b's
// forward — both run in the same workgroup with a __syncthreads where
// the inter-kernel dependency used to be.  Saves one ~4.5 us dispatch
// and the w2 re-staging (5000 floats/WG) the separate bwd kernel pays.
// Cost: the backward loses its `split` sibling-workgroup parallelism
// (grid = B, not B*split), so at small B the chip is underfilled.
// The backward LDS carve aliases the forward's dead buffers: total
// 5020 (w2s, shared by both phases — same [k*10+c]*25 weight layout)
// + 7168 floats = 47.7 KB/WG -> 3 WGs/CU.
__global__ void
__launch_bounds__(256)
net_fused_fwdbwd_kernel(NetIn in, GwPtrs prm, NetWs ws) {
  __shared__ __attribute__((aligned(16))) float w2s[N_C2K * 250 + N_C2K];
  __shared__ __attribute__((aligned(16))) float pool[7168];
  const int tid = threadIdx.x;
  const int B = in.B;
  const uint64_t seed = in.seed[0];
  // forward carve
  float* xs = pool;              // 784
  float* w1s = pool + 784;       // 260
  float* p1 = pool + 1048;       // 1440  (784+260=1044 -> pad to 1048)
  float* p2 = pool + 2488;       // 320
  float* d3 = pool + 2808;       // 50
  float* logits = pool + 2860;   // 10
  // backward carve (aliased onto the forward's dead buffers)
  float* gd2p = pool;            // 6080 (= 20 k-planes x 16 x 19)
  float* gp2 = pool + 6080;      // 320
  float* glg = pool + 6400;      // 10
  float* gd3 = pool + 6412;      // 50
  float* gh1 = pool + 6464;      // 50 -> 6514 (buffer 7168)
  const float sc = 1.f / B;      // dLoss == 1 by construction

  float lsum = 0.f;
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    const float lp_t = net_fwd_sample(
        b, tid, B, in.training, seed, 0, nullptr, 0u, in.x, prm.p[G_W1],
        prm.p[G_B1], prm.p[G_W2], prm.p[G_B2], prm.p[G_WF1], prm.p[G_BF1],
        prm.p[G_WF2], prm.p[G_BF2], in.tgt, ws.p1, ws.idx1, ws.m2, ws.p2,
        ws.idx2, ws.h1, ws.m3, ws.d3, ws.logp, xs, w1s, p1, w2s, p2, d3,
        logits);
    if (tid == 0) lsum += -lp_t / B;
    __syncthreads();  // fwd LDS dead + this block's global stashes visible
    net_bwd_sample(b, 0, 1, tid, B, in.training, sc, prm.p[G_WF1],
                   prm.p[G_WF2], in.tgt, ws.idx1, ws.m2, ws.idx2, ws.h1,
                   ws.m3, ws.logp, ws.glog, ws.gh1, ws.ga2, ws.ga1,
                   w2s, glg, gd3, gh1, gp2, gd2p);
    __syncthreads();  // bwd LDS dead before the next sample reuses pool
  }
  if (tid == 0) ws.loss_part[blockIdx.x] = lsum;
}

// Per-chunk partial weight gradients for all four layers in ONE launch
// (replaces 4 kernels + 8 memsets): grid.x walks tile segments
// [conv2 | conv1 | fc1 | fc2], grid.y is the batch chunk; partials land
// in part[chunk][21840] laid out exactly like the flat grad buffer
// (parameter order conv1.w,b conv2.w,b fc1.w,b fc2.w,b).
#define GW_TOTAL 21840
#define OFF_W1 0          // 250
#define OFF_B1 250        // 10
#define OFF_W2 260        // 5000
#define OFF_B2 5260       // 20
#define OFF_WF1 5280      // 16000
#define OFF_BF1 21280     // 50
#define OFF_WF2 21330     // 500
#define OFF_BF2 21830     // 10
#define T_CONV2 8         // conv2 tiles: 32-column slices of (c,r,s | bias)
#define T_CONV1 8         // conv1 sub-blocks: bands of 3 output rows
#define T_FC1 63          // ceil(16050/256)
#define T_FC2 2          // ceil(510/256)
#define GW_TILES (T_CONV2 + T_CONV1 + T_FC1 + T_FC2)  // in walk order
// conv1's 8 sub-blocks write disjoint 260-float slices: sub 0 to the
// canonical [OFF_W1,OFF_B1] region, subs 1-7 to an extension past
// GW_TOTAL; the combine kernel folds the extension back in.
#define GW_ROW (GW_TOTAL + (T_CONV1 - 1) * 260)

typedef float gw_f32x16 __attribute__((ext_vector_type(16)));
typedef float gw_f32x4 __attribute__((ext_vector_type(4)));

// conv2 weight gradient as an implicit GEMM on exact-fp32 MFMA
// (v_mfma_f32_32x32x2_f32; numerics are a k-ordered fmaf chain):
//   M = 20 output channels (rows 20..31 fed zeros),
//   N = 250 (c,r,s) columns + the bias as column 250 (B = ones),
//       cut into 8 tiles of 32 — ONE BLOCK PER COLUMN TILE, all 20
//       channels, so a chunk row stages p1 8 x (<= 3 of 10 planes)
//       instead of 10-20 x the whole plane,
//   K = (b, oh, ow), 64 per sample, split over the 4 waves: wave w owns
//       positions 16w..16w+15.  K order inside a wave is free as long as
//       A and B agree, so MFMA step j (0..7) of lane half h is position
//       16w + 8h + j, i.e. (oh, ow) = (2w + h, j): the A operand is 8
//       CONTIGUOUS ga2 floats per lane (two float4 loads straight from
//       global, prefetched one sample ahead) and the B operand 8
//       contiguous LDS floats at a per-lane column base.
// Operand lane map (32x32x2): lane l gives A[row l&31][k l>>5] and
// B[k l>>5][col l&31]; D[row (reg&3) + 8*(reg>>2) + 4*(l>>5)][col l&31].
// One accumulator tile per wave is enough: the 32x32x2 dependent-chain
// latency equals its issue interval (64 clk).  The four K-slices are
// summed once per chunk through LDS in a fixed order (deterministic).
// Every accumulator index is compile-time (a runtime index spilled to
// scratch and tripled this kernel once — r2 ledger).
static_assert(T_CONV2 * 32 >= 251, "conv2 gw column tiles cover 250 + bias");
template <bool SC1 = false>
__device__ __forceinline__ void net_gw_conv2_mfma(
    int nt, int tid, int b0, int b1, float* __restrict__ my,
    const float* __restrict__ p1_ws, const float* __restrict__ ga2_ws) {
  __shared__ __attribute__((aligned(16))) float sp1[2][3 * 144];
  __shared__ float red[4][N_C2K * 32];
  const int lane = tid & 63, w = tid >> 6;
  const int col = lane & 31, h = lane >> 5;
  const int n = nt * 32 + col;
  // 32 consecutive columns touch at most 3 input channels
  const int c_lo = (nt * 32) / 25;
  const int c_hi = min(N_C1K - 1, (nt * 32 + 31) / 25);
  const int nst4 = (c_hi - c_lo + 1) * 36;  // float4s to stage (<= 108)
  // per-lane im2col base: c*144 + (oh + r)*12 + (ow + s), oh = 2w + h
  int base = (2 * w + h) * 12;
  if (n < 250) base += (n / 25 - c_lo) * 144 + ((n % 25) / 5) * 12 + n % 5;
  const float bfix = (n == 250) ? 1.f : 0.f;  // bias column / padding
  const int aoff = col * 64 + 16 * w + 8 * h;
  gw_f32x16 acc;
  #pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0;
  // b0 < b1 guard: ceil-rounded chunk counts leave EMPTY tail rows for
  // non-divisible B (e.g. B=100, nch=16, bchunk=7 -> row 15 starts at
  // sample 105); such a row must touch no memory and flush zeros.
  if (b0 < b1) {
    if (tid < nst4)
      reinterpret_cast<float4*>(sp1[0])[tid] =
          reinterpret_cast<const float4*>(
              p1_ws + (int64_t)b0 * N_P1 + c_lo * 144)[tid];
    if (col < N_C2K) {
      const float4* ap = reinterpret_cast<const float4*>(
          ga2_ws + (int64_t)b0 * N_A2 + aoff);
      a0 = ap[0];
      a1 = ap[1];
    }
  }
  __syncthreads();
  for (int b = b0; b < b1; ++b) {
    const int cur = (b - b0) & 1;
    // next sample: global loads issued before the MFMAs, LDS write after
    const bool more = b + 1 < b1;
    float4 st = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 n0 = st, n1 = st;
    if (more) {
      if (tid < nst4)
        st = reinterpret_cast<const float4*>(
            p1_ws + (int64_t)(b + 1) * N_P1 + c_lo * 144)[tid];
      if (col < N_C2K) {
        const float4* ap = reinterpret_cast<const float4*>(
            ga2_ws + (int64_t)(b + 1) * N_A2 + aoff);
        n0 = ap[0];
        n1 = ap[1];
      }
    }
    const float* bp = sp1[cur] + base;
    float bv[8];
    #pragma unroll
    for (int j = 0; j < 8; ++j) bv[j] = (n < 250) ? bp[j] : bfix;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, bv[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, bv[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.z, bv[2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.w, bv[3], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, bv[4], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, bv[5], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.z, bv[6], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.w, bv[7], acc, 0, 0, 0);
    if (more && tid < nst4)
      reinterpret_cast<float4*>(sp1[cur ^ 1])[tid] = st;
    a0 = n0;
    a1 = n1;
    __syncthreads();
  }
  // rows (channels) 0..19 of this wave's K-slice -> red[w][k][col]
  #pragma unroll
  for (int reg = 0; reg < 12; ++reg) {
    const int k = (reg & 3) + 8 * (reg >> 2) + 4 * h;
    if (reg < 8 || h == 0) red[w][k * 32 + col] = acc[reg];
  }
  __syncthreads();
  for (int i = tid; i < N_C2K * 32; i += 256) {
    const int k = i >> 5, nn = nt * 32 + (i & 31);
    const float v = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
    if (nn < 250)
      gw_st<SC1>(my + OFF_W2 + k * 250 + nn, v);
    else if (nn == 250)
      gw_st<SC1>(my + OFF_B2 + k, v);
  }
}

// conv1 weight gradient on exact-fp32 MFMA (v_mfma_f32_16x16x4_f32):
//   M = 10 output channels (pad 16), N = 25 (r,s) + the bias as column
//   25 (B = ones), pad 32 = two 16-wide tiles sharing the A operand,
//   K = (b, oh, ow).  Sub-block `sub` of T_CONV1 owns a band of
//   24/T_CONV1 output rows; inside it the (sample, row) pairs are dealt
//   round-robin to the 4 waves.  One row = 24 positions = 6 MFMA steps:
//   step j of lane group q = l>>4 is ow = 6q + j, so each lane reads 6
//   contiguous ga1 floats (A) and 6 contiguous x floats per tile (B)
//   straight from global — these re-reads are L1 hits (r2 ledger), and
//   there is no barrier in the K loop.
// Lane map (16x16x4): A[row l&15][k l>>4], B[k l>>4][col l&15];
// D[row 4*(l>>4) + reg][col l&15].  Two independent accumulator tiles
// per wave cover the 40-clk dependent latency (32-clk issue).
template <bool SC1 = false>
__device__ __forceinline__ void net_gw_conv1_mfma(
    int sub, int tid, int b0, int b1, float* __restrict__ my,
    const float* __restrict__ x, const float* __restrict__ ga1_ws) {
  __shared__ float red[4][260];
  const int lane = tid & 63, w = tid >> 6;
  const int m = lane & 15, q = lane >> 4;
  constexpr int rows = 24 / T_CONV1;
  static_assert(rows * T_CONV1 == 24, "conv1 bands tile the 24 rows");
  const int oh0 = sub * rows;
  const int n1 = 16 + m;  // second tile: 16..24 weights, 25 bias, 26.. pad
  const int xo0 = (m / 5) * 28 + m % 5 + 6 * q;
  const int xo1 = (n1 < 25) ? (n1 / 5) * 28 + n1 % 5 + 6 * q : 0;
  const float bfix = (n1 == 25) ? 1.f : 0.f;
  const int ao = m * 576 + 6 * q;
  gw_f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  const int ntask = (b1 > b0) ? (b1 - b0) * rows : 0;
  for (int t = w; t < ntask; t += 4) {
    const int bb = t / rows;
    const int b = b0 + bb, oh = oh0 + (t - bb * rows);
    float av[6], v0[6], v1[6];
    if (m < N_C1K) {
      const float2* gp = reinterpret_cast<const float2*>(
          ga1_ws + (int64_t)b * N_A1 + ao + oh * 24);
      const float2 g0 = gp[0], g1 = gp[1], g2 = gp[2];
      av[0] = g0.x; av[1] = g0.y; av[2] = g1.x;
      av[3] = g1.y; av[4] = g2.x; av[5] = g2.y;
    } else {
      #pragma unroll
      for (int j = 0; j < 6; ++j) av[j] = 0.f;
    }
    const float* xp = x + (int64_t)b * 784 + oh * 28;
    #pragma unroll
    for (int j = 0; j < 6; ++j) {
      v0[j] = xp[xo0 + j];
      v1[j] = (n1 < 25) ? xp[xo1 + j] : bfix;
    }
    #pragma unroll
    for (int j = 0; j < 6; ++j) {
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], v0[j], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], v1[j], acc1, 0, 0, 0);
    }
  }
  #pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int k = 4 * q + reg;
    if (k < N_C1K) {
      red[w][k * 25 + m] = acc0[reg];
      if (n1 < 25) red[w][k * 25 + n1] = acc1[reg];
      if (n1 == 25) red[w][250 + k] = acc1[reg];
    }
  }
  __syncthreads();
  // sub 0 writes the canonical region, subs 1.. the extension rows
  float* dst = (sub == 0) ? (my + OFF_W1)
                          : (my + GW_TOTAL + (sub - 1) * 260);
  for (int i = tid; i < 260; i += 256)
    gw_st<SC1>(dst + i,
               (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]));
}

// One (tile, batch-chunk) partial weight-gradient reduction.  Tiles
// walk [conv2 x8 | conv1 x8 | fc1 | fc2]; partials land in my[GW_ROW]
// laid out like the flat grad buffer.  Shared by net_gw_partial_kernel
// and the single-launch net_step_kernel.
template <bool SC1 = false>
__device__ __forceinline__ void net_gw_tile(
    int tile, int tid, int b0, int b1,
    float* __restrict__ my,
    const float* __restrict__ x,
    const float* __restrict__ p1_ws,
    const float* __restrict__ p2_ws,
    const float* __restrict__ d3_ws,
    const float* __restrict__ ga1_ws,
    const float* __restrict__ ga2_ws,
    const float* __restrict__ gh1_ws,
    const float* __restrict__ glog_ws) {
  if (tile < T_CONV2) {  // conv2: gw [20][10][5][5] + gb [20]
    // one code path for every chunk size: a block is one 32-column
    // slice of the implicit GEMM over ALL 20 output channels
    net_gw_conv2_mfma<SC1>(tile, tid, b0, b1, my, p1_ws, ga2_ws);
    return;
  }
  tile -= T_CONV2;
  if (tile < T_CONV1) {  // conv1: gw [10][1][5][5] + gb [10]
    // K (the 24 output rows x batch chunk) is split over T_CONV1
    // sub-blocks; sub 0 writes the canonical region, subs 1.. the
    // extension rows, which the combine folds.
    net_gw_conv1_mfma<SC1>(tile, tid, b0, b1, my, x, ga1_ws);
    return;
  }
  tile -= T_CONV1;
  if (tile < T_FC1) {  // fc1: gw [50][320] + gb [50]
    const int i = tile * 256 + tid;
    if (i < 16050) {
      float acc = 0.f;
      if (i < 16000) {
        const int n = i / N_P2, k = i % N_P2;
        float ae = 0.f, ao = 0.f;
        int b = b0;
        for (; b + 1 < b1; b += 2) {
          ae += gh1_ws[(int64_t)b * N_H1 + n] *
                p2_ws[(int64_t)b * N_P2 + k];
          ao += gh1_ws[(int64_t)(b + 1) * N_H1 + n] *
                p2_ws[(int64_t)(b + 1) * N_P2 + k];
        }
        if (b < b1)
          ae += gh1_ws[(int64_t)b * N_H1 + n] *
                p2_ws[(int64_t)b * N_P2 + k];
        acc = ae + ao;
        gw_st<SC1>(my + OFF_WF1 + i, acc);
      } else {
        const int n = i - 16000;
        for (int b = b0; b < b1; ++b)
          acc += gh1_ws[(int64_t)b * N_H1 + n];
        gw_st<SC1>(my + OFF_BF1 + n, acc);
      }
    }
    return;
  }
  tile -= T_FC1;
  {  // fc2: gw [10][50] + gb [10]
    const int i = tile * 256 + tid;
    if (i < 510) {
      float acc = 0.f;
      if (i < 500) {
        const int n = i / N_H1, k = i % N_H1;
        for (int b = b0; b < b1; ++b)
          acc += glog_ws[(int64_t)b * N_CLS + n] *
                 d3_ws[(int64_t)b * N_H1 + k];
        gw_st<SC1>(my + OFF_WF2 + i, acc);
      } else {
        const int n = i - 500;
        for (int b = b0; b < b1; ++b)
          acc += glog_ws[(int64_t)b * N_CLS + n];
        gw_st<SC1>(my + OFF_BF2 + n, acc);
      }
    }
  }
}

__global__ void __launch_bounds__(256)
net_gw_partial_kernel(// pointer by pointer: with NetWs by value this kernel
                      // measured 0.2-0.7 us slower
                      // (profiles/net_fused_args.md)
                      const float* __restrict__ x,
                      const float* __restrict__ p1_ws,
                      const float* __restrict__ p2_ws,
                      const float* __restrict__ d3_ws,
                      const float* __restrict__ ga1_ws,
                      const float* __restrict__ ga2_ws,
                      const float* __restrict__ gh1_ws,
                      const float* __restrict__ glog_ws,
                      float* __restrict__ part,  // [max chunk][GW_ROW]
                      int B, int bchunk, int bchunk1, int bchunk2,
                      int nch, int nch1, int nch2, int tile_base) {
  // conv1/conv2 run at their own chunk counts (they are the straggler
  // families at small B); gridDim.y = max of the three, families idle
  // on the rows beyond their own count (idle blocks are
  // launch-granularity free)
  const int tile = blockIdx.x + tile_base;
  const bool c2 = tile < T_CONV2;
  const bool c1 = tile >= T_CONV2 && tile < T_CONV2 + T_CONV1;
  if ((int)blockIdx.y >= (c2 ? nch2 : c1 ? nch1 : nch)) return;
  const int bc = c2 ? bchunk2 : c1 ? bchunk1 : bchunk;
  net_gw_tile(tile, threadIdx.x, (int)blockIdx.y * bc,
              min(B, ((int)blockIdx.y + 1) * bc),
              part + (int64_t)blockIdx.y * GW_ROW,
              x, p1_ws, p2_ws, d3_ws, ga1_ws, ga2_ws, gh1_ws, glog_ws);
}

// combine: grads[i] = sum over chunks of part[c][i], written through
// the 8 per-parameter pointers (which may alias one flat buffer).
// sum flat-grad element i over the nch chunk rows (+ conv1 extension)
template <bool SC1 = false>
__device__ __forceinline__ float net_gw_combine_elem(
    int i, int nch, int nch1, int nch2,
    const float* __restrict__ part) {
  // four independent accumulator chains: the single 32-deep
  // load+add chain was latency-bound (VALUBusy ~0, profiles/).
  // nch1/nch2: the conv1/conv2 families may run at their OWN chunk
  // counts (they are the gw stragglers at small B; more chunks = more
  // parallelism there without paying their fold cost on every other
  // family, which is what made a GLOBAL chunk increase lose) —
  // conv1-region elements (i < 260, extensions included) fold nch1
  // rows, conv2-region elements nch2 rows, everything else nch.
  const int n = i < 260 ? nch1
              : (i >= OFF_W2 && i < OFF_WF1) ? nch2 : nch;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  int c = 0;
  for (; c + 3 < n; c += 4) {
    a0 += gw_ld<SC1>(part + (int64_t)c * GW_ROW + i);
    a1 += gw_ld<SC1>(part + (int64_t)(c + 1) * GW_ROW + i);
    a2 += gw_ld<SC1>(part + (int64_t)(c + 2) * GW_ROW + i);
    a3 += gw_ld<SC1>(part + (int64_t)(c + 3) * GW_ROW + i);
  }
  for (; c < n; ++c) a0 += gw_ld<SC1>(part + (int64_t)c * GW_ROW + i);
  if (i < 260) {  // conv1 sub-block extension rows (see GW_ROW)
    // fully unrolled over the 7 rows — a runtime-bound loop here cost
    // the combine 50% (8.1 -> 12.2 us, r2 ledger)
    static_assert(T_CONV1 == 8, "extension fold is unrolled for 7 rows");
    for (int c2 = 0; c2 < nch1; ++c2) {
      const float* ext = part + (int64_t)c2 * GW_ROW + GW_TOTAL;
      a0 += gw_ld<SC1>(ext + i) + gw_ld<SC1>(ext + 4 * 260 + i);
      a1 += gw_ld<SC1>(ext + 260 + i) + gw_ld<SC1>(ext + 5 * 260 + i);
      a2 += gw_ld<SC1>(ext + 2 * 260 + i) + gw_ld<SC1>(ext + 6 * 260 + i);
      a3 += gw_ld<SC1>(ext + 3 * 260 + i);
    }
  }
  return (a0 + a1) + (a2 + a3);
}

__device__ __forceinline__ int net_gw_tensor_of(int i, const int* off) {
  int t = 0;
  while (i >= off[t + 1]) ++t;
  return t;
}

// ---------------------------------------------------------------------------
// The combine dispatch: grads[i] = sum over chunk rows of part[c][i],
// optionally followed by the SGD+momentum update, plus the loss
// finalise and the seed advance.  Its work is tiny (about 2 MB read), so
// its time is the number of DEPENDENT memory round trips on its longest
// path.  Every block therefore issues all of its loads (partial rows,
// momentum, parameter) before its first wait: the row loops have
// compile-time bounds, and a row past the family's chunk count is
// CLAMPED to the last live row and its value replaced by 0 (a branch
// around a load makes hipcc wait per load; a clamped load hits the line
// a neighbour already fetched).  Rows >= n are never read.
//
// Grid (net_gw_combine_grid): [conv1 x GW_CB_C1 | loss | seed | main].
//   conv1 block: 16 consecutive elements of [0,260) x 16 row groups.
//     An element sums nch1 * T_CONV1 slots (sub 0 in the canonical
//     region, subs 1-7 in the extension); group r takes slot r & 7 of
//     chunk rows 2k + (r >> 3), k = 0..15.  The element index is
//     fastest across lanes, so 16 lanes read one 64-byte segment.
//   loss block: sums loss_part; seed block: advances the seed.  On
//     their own so that no gradient element waits behind them, nor the
//     loss behind the seed's round trip.
//   main block: elements [260, GW_TOTAL), 4 lanes each; lane q takes
//     rows q + 4k, k = 0..7.
// All sums run in a fixed order (no atomics): deterministic.
#define GW_MAX_CH 32      // rows of the part workspace
#define GW_CB_C1 ((260 + 15) / 16)
#define GW_CB_MAIN (((GW_TOTAL - 260) * 4 + 255) / 256)
static_assert(T_CONV1 == 8 && GW_MAX_CH == 32,
              "conv1 block: 16 groups x 16 rows cover 32 chunks x 8 slots");

static inline dim3 net_gw_combine_grid() {
  return dim3(GW_CB_C1 + 2 + GW_CB_MAIN);
}

// Pointer of flat-grad element i in its own tensor (null when the
// tensor's pointer is null), for i in the conv1 region (C1) or past it:
// compile-time comparisons, constant indices.  gw_pin keeps a pointer
// in scalar registers; left alone, hipcc turns the select chain back
// into one indexed load from the kernarg segment, a memory round trip
// that every later load waits for.  The result is typed as global
// memory, which the pin would otherwise hide (flat instead of global
// loads and stores).
typedef __attribute__((address_space(1))) float gw_gfloat;

__device__ __forceinline__ gw_gfloat* gw_pin(float* q) {
  asm volatile("" : "+s"(q));
  return (gw_gfloat*)q;
}

template <bool C1>
__device__ __forceinline__ gw_gfloat* net_gw_ptr_of(const GwPtrs& p,
                                                    int i) {
  gw_gfloat* b;
  int o;
  if (C1) {
    gw_gfloat* const w1 = gw_pin(p.p[0]), * const b1 = gw_pin(p.p[1]);
    b = i < OFF_B1 ? w1 : b1;
    o = i < OFF_B1 ? OFF_W1 : OFF_B1;
  } else {
    gw_gfloat* const w2 = gw_pin(p.p[2]), * const b2 = gw_pin(p.p[3]);
    gw_gfloat* const wf1 = gw_pin(p.p[4]), * const bf1 = gw_pin(p.p[5]);
    gw_gfloat* const wf2 = gw_pin(p.p[6]), * const bf2 = gw_pin(p.p[7]);
    b = w2, o = OFF_W2;
    if (i >= OFF_B2) b = b2, o = OFF_B2;
    if (i >= OFF_WF1) b = wf1, o = OFF_WF1;
    if (i >= OFF_BF1) b = bf1, o = OFF_BF1;
    if (i >= OFF_WF2) b = wf2, o = OFF_WF2;
    if (i >= OFF_BF2) b = bf2, o = OFF_BF2;
  }
  return b ? b + (i - o) : nullptr;
}

// one output element: its three addresses, and the momentum and
// parameter values, whose loads are issued here, ahead of the row loads
struct GwElem { gw_gfloat* g; gw_gfloat* prm; gw_gfloat* buf; float b, p; };

template <bool SGD, bool C1>
__device__ __forceinline__ GwElem net_gw_elem_open(
    int i, const GwPtrs& g, const GwPtrs& prm, const GwPtrs& buf) {
  GwElem e{net_gw_ptr_of<C1>(g, i), nullptr, nullptr, 0.f, 0.f};
  if (SGD) {
    e.prm = net_gw_ptr_of<C1>(prm, i);
    e.buf = net_gw_ptr_of<C1>(buf, i);
    e.p = *e.prm;
    e.b = *(e.buf ? e.buf : e.prm);  // no buffer: any valid address
    // the loads stay HERE: without this, hipcc sinks them into the
    // branch of the one lane that stores, behind the row loads' wait
    asm volatile("" ::: "memory");
  }
  return e;
}

// write the grad; SGD: v = mu*buf + g; buf = v; prm -= lr*v, exactly
// like sgd_step_kernel (a null buffer means no momentum)
template <bool SGD>
__device__ __forceinline__ void net_gw_elem_close(const GwElem& e, float acc,
                                                  float lr, float mu) {
  *e.g = acc;
  if (SGD) {
    float v = acc;
    if (e.buf) {
      v = mu * e.b + acc;
      *e.buf = v;
    }
    *e.prm = e.p - lr * v;
  }
}

// sum the nblk_fwd per-block loss partials of the forward kernel into
// loss_out (null loss_part: legacy mode, nothing to do)
__device__ __forceinline__ void net_gw_loss_block(
    const float* __restrict__ loss_part, float* __restrict__ loss_out,
    int nblk_fwd, float* sh) {
  const int tid = threadIdx.x;
  if (loss_part) {  // block-uniform
    float v = 0.f;
    for (int base = 0; base < nblk_fwd; base += 4 * 256) {
      float t[4];
      #pragma unroll
      for (int k = 0; k < 4; ++k)
        t[k] = loss_part[min(base + k * 256 + tid, nblk_fwd - 1)];
      #pragma unroll
      for (int k = 0; k < 4; ++k)
        v += (base + k * 256 + tid < nblk_fwd) ? t[k] : 0.f;
    }
    v = block_sum(v, sh);
    if (tid == 0) *loss_out = v;
  }
}

template <bool SGD>
__device__ __forceinline__ void net_gw_combine_body(
    const float* __restrict__ part, const GwPtrs& g, const GwPtrs& prm,
    const GwPtrs& buf, int nch, int nch1, int nch2, float lr, float mu,
    const float* __restrict__ loss_part, float* __restrict__ loss_out,
    int nblk_fwd, unsigned long long* seed_bump) {
  __shared__ float sh[NWAVE * 16];
  const int tid = threadIdx.x, blk = blockIdx.x;
  if (blk == GW_CB_C1) {
    net_gw_loss_block(loss_part, loss_out, nblk_fwd, sh);
    return;
  }
  if (blk == GW_CB_C1 + 1) {
    // advance the dropout seed for the NEXT step.  The convention is
    // bump-AFTER everywhere: the step consumes the current seed, the
    // combine advances it; a null pointer leaves it alone.
    if (tid == 0 && seed_bump) *seed_bump += SEED_INC;
    return;
  }
  if (blk < GW_CB_C1) {  // conv1: 16 elements x 16 row groups
    const int el = tid & 15, r = tid >> 4;
    const int i = min(blk * 16 + el, 259);
    const bool live = tid < 16 && blk * 16 + el < 260;
    const GwElem e = net_gw_elem_open<SGD, true>(i, g, prm, buf);
    const int slot = r & 7;
    const int col = slot == 0 ? i : GW_TOTAL + (slot - 1) * 260 + i;
    float t[16];
    #pragma unroll
    for (int k = 0; k < 16; ++k)
      t[k] = part[min(2 * k + (r >> 3), nch1 - 1) * GW_ROW + col];
    #pragma unroll
    for (int k = 0; k < 16; ++k)
      if (2 * k + (r >> 3) >= nch1) t[k] = 0.f;
    float acc = 0.f;
    #pragma unroll
    for (int k = 0; k < 16; k += 8) {
      const float t8[8] = {t[k], t[k + 1], t[k + 2], t[k + 3],
                           t[k + 4], t[k + 5], t[k + 6], t[k + 7]};
      acc += tree8(t8);
    }
    acc += __shfl_xor(acc, 16, 64);  // the wave's 4 groups
    acc += __shfl_xor(acc, 32, 64);
    if ((tid & 63) < 16) sh[(tid >> 6) * 16 + el] = acc;
    __syncthreads();
    if (live)
      net_gw_elem_close<SGD>(
          e, (sh[el] + sh[16 + el]) + (sh[32 + el] + sh[48 + el]), lr, mu);
    return;
  }
  // fc and conv2 regions: 4 lanes per element
  const int t4 = (blk - GW_CB_C1 - 2) * 256 + tid;
  const int q = t4 & 3;
  const bool live = q == 0 && OFF_W2 + (t4 >> 2) < GW_TOTAL;
  const int i = min(OFF_W2 + (t4 >> 2), GW_TOTAL - 1);
  const GwElem e = net_gw_elem_open<SGD, false>(i, g, prm, buf);
  const int n = i < OFF_WF1 ? nch2 : nch;
  float t[GW_MAX_CH / 4];
  #pragma unroll
  for (int k = 0; k < GW_MAX_CH / 4; ++k)
    t[k] = part[min(q + 4 * k, n - 1) * GW_ROW + i];
  #pragma unroll
  for (int k = 0; k < GW_MAX_CH / 4; ++k)
    if (q + 4 * k >= n) t[k] = 0.f;
  static_assert(GW_MAX_CH / 4 == 8, "the lane sum is one tree8");
  float acc = tree8(t);
  acc += __shfl_xor(acc, 1, 4);
  acc += __shfl_xor(acc, 2, 4);
  if (live) net_gw_elem_close<SGD>(e, acc, lr, mu);
}

// combine alone (the world>1 path: the all-reduce sits between it and
// the optimizer step)
__global__ void __launch_bounds__(256)
net_gw_combine_kernel(const float* __restrict__ part, GwPtrs g, int nch,
                      int nch1, int nch2,
                      const float* __restrict__ loss_part,
                      float* __restrict__ loss_out, int nblk_fwd,
                      unsigned long long* seed_bump) {
  net_gw_combine_body<false>(part, g, g, g, nch, nch1, nch2, 0.f, 0.f,
                             loss_part, loss_out, nblk_fwd, seed_bump);
}

// combine + SGD in one dispatch (single-GPU training: there is no
// gradient all-reduce between combine and the optimizer step, so the
// dispatch of a separate sgd_step_kernel is pure overhead).  Writes the
// grad (so .grad stays inspectable), updates the momentum buffer and
// the parameter exactly like sgd_step_kernel.
__global__ void __launch_bounds__(256)
net_gw_combine_sgd_kernel(const float* __restrict__ part, GwPtrs g,
                          GwPtrs prm, GwPtrs buf, int nch, int nch1,
                          int nch2, float lr, float mu,
                          const float* __restrict__ loss_part,
                          float* __restrict__ loss_out, int nblk_fwd,
                          unsigned long long* seed_bump) {
  net_gw_combine_body<true>(part, g, prm, buf, nch, nch1, nch2, lr, mu,
                            loss_part, loss_out, nblk_fwd, seed_bump);
}

// ---------------------------------------------------------------------------
// In-launch gw fold (r2): the combine dispatch is pure latency (~10 us at
// B=128 — 86 tiny blocks, an L2-chain fold of 1.4 MB of partials), so this
// variant of the partial kernel deletes it: the LAST-ARRIVING block of each
// tile column folds the region its column wrote (and, DO_SGD, applies the
// momentum update), using the split-K last-arriver recipe from the CDNA
// guide (G16): every block drains vmcnt + __syncthreads, lane 0 issues an
// agent-scope RELEASE fence, restates the vmcnt wait, THEN takes a relaxed
// agent-scope ticket; the block that draws target-1 acquires (agent) and
// reads every row with plain loads.  Fold regions are per COLUMN (what the
// column's own blocks wrote), so counter==target implies the region's rows
// are all visible:
//   conv2 column t  -> columns 32t..32t+31 of (c,r,s | bias), all 20
//                      output channels
//   conv1 family    -> ONE counter over all T_CONV1*nch blocks (its
//                      sub-blocks share the 260 outputs via extension rows,
//                      so no single column's completion suffices)
//   fc1/fc2 column j -> its 256-element flat slice
// Each fold runs as soon as ITS column's blocks are done — overlapped with
// the other families still computing — so the only exposed cost is the
// straggler family's own (tiny) fold.
__device__ __forceinline__ void net_gw_fold_one(
    int i, int nch, const float* __restrict__ part,
    const GwPtrs& g, const GwPtrs& prm, const GwPtrs& buf, float lr,
    float mu, bool do_sgd) {
  const int off[9] = {OFF_W1, OFF_B1, OFF_W2, OFF_B2, OFF_WF1, OFF_BF1,
                      OFF_WF2, OFF_BF2, GW_TOTAL};
  const float acc = net_gw_combine_elem<true>(i, nch, nch, nch, part);
  const int t = net_gw_tensor_of(i, off);
  const int64_t j = i - off[t];
  g.p[t][j] = acc;
  if (do_sgd) {
    float v = acc;
    if (buf.p[t]) {
      v = mu * buf.p[t][j] + acc;
      buf.p[t][j] = v;
    }
    prm.p[t][j] -= lr * v;
  }
}

__device__ __forceinline__ void net_gw_fold_range(
    int i0, int i1, int nch, const float* __restrict__ part,
    const GwPtrs& g, const GwPtrs& prm, const GwPtrs& buf, float lr,
    float mu, bool do_sgd) {
  for (int i = i0 + (int)threadIdx.x; i < i1; i += 256)
    net_gw_fold_one(i, nch, part, g, prm, buf, lr, mu, do_sgd);
}

template <bool DO_SGD>
__global__ void __launch_bounds__(256)
net_gw_partial_fold_kernel(const float* __restrict__ x, NetWs ws, int B,
                           int bchunk,
                           GwPtrs g, GwPtrs prm, GwPtrs buf, float lr,
                           float mu, const float* __restrict__ loss_part,
                           float* __restrict__ loss_out, int nblk_fwd,
                           unsigned long long* seed_bump,
                           unsigned int* __restrict__ cnt) {
  const int b0 = blockIdx.y * bchunk;
  float* __restrict__ part = ws.part;
  net_gw_tile<true>(blockIdx.x, threadIdx.x, b0, min(B, b0 + bchunk),
                    part + (int64_t)blockIdx.y * GW_ROW, x, ws.p1, ws.p2,
                    ws.d3, ws.ga1, ws.ga2, ws.gh1, ws.glog);
  // ---- last-arriver ticket, FENCE-FREE: the tile wrote its partials
  // with sc1 stores (already at the coherence point once vmcnt
  // retires), so the ticket needs only the vmcnt drain before it and
  // the reducer reads the rows back with sc1 loads.  No buffer_wbl2 /
  // buffer_inv anywhere — the concurrent tile blocks keep their
  // L1/L2-resident activations (the fenced variant cost 23-28%).
  const int nch = (int)gridDim.y;
  const int xcol = (int)blockIdx.x;
  const bool conv1_fam = (xcol >= T_CONV2 && xcol < T_CONV2 + T_CONV1);
  const int ci = conv1_fam ? T_CONV2 : xcol;
  const unsigned target =
      conv1_fam ? (unsigned)(T_CONV1 * nch) : (unsigned)nch;
  __shared__ unsigned s_tk;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0)
    s_tk = __hip_atomic_fetch_add(&cnt[ci], 1u, __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  if (s_tk != target - 1) return;  // not the last arriver of this region
  if (threadIdx.x == 0)
    __hip_atomic_store(&cnt[ci], 0u, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);  // re-arm for next step
  __syncthreads();
  if (xcol < T_CONV2) {  // conv2: this column's 32-wide slice, all k
    for (int e = (int)threadIdx.x; e < N_C2K * 32; e += 256) {
      const int k = e >> 5, nn = xcol * 32 + (e & 31);
      if (nn > 250) continue;
      const int i = nn < 250 ? OFF_W2 + k * 250 + nn : OFF_B2 + k;
      net_gw_fold_one(i, nch, part, g, prm, buf, lr, mu, DO_SGD);
    }
    return;
  }
  if (conv1_fam) {  // conv1: canonical 260 + extension rows
    net_gw_fold_range(0, 260, nch, part, g, prm, buf, lr, mu,
                      DO_SGD);
    return;
  }
  if (xcol < T_CONV2 + T_CONV1 + T_FC1) {  // fc1 column slice
    const int i0 = OFF_WF1 + (xcol - (T_CONV2 + T_CONV1)) * 256;
    net_gw_fold_range(i0, min(OFF_WF1 + 16050, i0 + 256), nch, part, g, prm, buf, lr, mu, DO_SGD);
    return;
  }
  // fc2 column slice; the last column also finalizes the loss partials
  // and advances the dropout seed (wave 0 only — no extra LDS).
  const int i0 = OFF_WF2 + (xcol - (T_CONV2 + T_CONV1 + T_FC1)) * 256;
  net_gw_fold_range(i0, min(OFF_WF2 + 510, i0 + 256), nch, part,
                    g, prm, buf, lr, mu, DO_SGD);
  if (xcol == GW_TILES - 1 && threadIdx.x < 64) {
    if (loss_part) {
      float v = 0.f;
      for (int i = threadIdx.x; i < nblk_fwd; i += 64) v += loss_part[i];
      #pragma unroll
      for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s, 64);
      if (threadIdx.x == 0 && loss_out) *loss_out = v;
    }
    if (threadIdx.x == 0 && seed_bump)
      *seed_bump += SEED_INC;
  }
}

// ===========================================================================
// Single-launch training step (cooperative kernel).
//
// The 6-dispatch step (prologue, fwd, bwd, gw-partial, combine, sgd)
// pays a ~4.5 us device dispatch floor per kernel at the reference's
// batch sizes (rocprof, profiles/).  This kernel runs the WHOLE step —
// forward, data backward, weight-gradient reduction, combine and the
// SGD+momentum update — in ONE hipLaunchCooperativeKernel dispatch,
// with cooperative-groups grid barriers between phases.  The per-phase
// work is the same shared __device__ code as the modular kernels
// (net_fwd_sample / net_bwd_sample / net_gw_tile / net_gw_combine_elem)
// so numerics are identical by construction.
//
// The loss is accumulated per-workgroup (loss_part, no atomics and no
// pre-zeroing) and summed into loss_out by workgroup 0 in the last
// phase, which also advances the device dropout seed for the NEXT step
// (replacing the step-prologue kernel; hipGraph-replay safe).
//
// When do_sgd == 0 the kernel stops after writing grads (the DP path:
// host runs the flat-gradient all-reduce, then sgd_step_kernel).
// ===========================================================================
namespace cg = cooperative_groups;

__global__ void __launch_bounds__(256)
net_step_kernel(
    // (with NetWs by value its pointers are all loaded at entry and held:
    // at 256 VGPRs and occupancy 1 that spilled SGPRs to VGPR lanes)
    const float* __restrict__ x,
    const int64_t* __restrict__ tgt,
    const float* __restrict__ gl,
    float* __restrict__ p1_ws, uint8_t* __restrict__ idx1_ws,
    uint8_t* __restrict__ m2_ws, float* __restrict__ p2_ws,
    uint8_t* __restrict__ idx2_ws, float* __restrict__ h1_ws,
    uint8_t* __restrict__ m3_ws, float* __restrict__ d3_ws,
    float* __restrict__ logp_ws, float* __restrict__ glog_ws,
    float* __restrict__ gh1_ws, float* __restrict__ ga2_ws,
    float* __restrict__ ga1_ws, float* __restrict__ part,
    float* __restrict__ loss_part,    // [gridDim.x]
    float* __restrict__ loss_out,     // scalar
    unsigned long long* __restrict__ seed_p,
    GwPtrs prm, GwPtrs grd, GwPtrs buf,
    float lr, float mu, int do_sgd,
    int B, int training, int split, int bchunk, int nch) {
  // LDS union: bwd carve (11,872 floats) reused by the fwd carve
  // (7,884) and the final-phase reduction scratch; phases are
  // separated by grid barriers.
  __shared__ __attribute__((aligned(16))) float smem[12192];
  float* xs = smem;             // 784
  float* w1s = xs + 784;        // 260
  float* p1 = w1s + 260;        // 1440
  float* w2s = p1 + 1440;       // 5020 (fwd: w2+b2)
  float* p2 = w2s + 5020;       // 320
  float* d3 = p2 + 320;         // 50
  float* logits = d3 + 50;      // 10
  float* b_w2s = smem;          // 5000 (bwd: w2 only)
  float* b_glg = smem + 5008;   // 10
  float* b_gd3 = smem + 5024;   // 50
  float* b_gh1 = smem + 5088;   // 50
  float* b_gp2 = smem + 5152;   // 320
  float* b_gd2p = smem + 5472;  // 6080 (20 x 16 x 19) -> 11552
  const int tid = threadIdx.x;
  const int wg = blockIdx.x, nblk = gridDim.x;
  cg::grid_group grid = cg::this_grid();

  const float* w1 = prm.p[G_W1]; const float* b1 = prm.p[G_B1];
  const float* w2 = prm.p[G_W2]; const float* b2 = prm.p[G_B2];
  const float* wf1 = prm.p[G_WF1]; const float* bf1 = prm.p[G_BF1];
  const float* wf2 = prm.p[G_WF2]; const float* bf2 = prm.p[G_BF2];
  const uint64_t seed = seed_p[0];

  // ---- phase 1: forward ------------------------------------------------
  float lsum = 0.f;
  for (int b = wg; b < B; b += nblk) {
    const float lp_t = net_fwd_sample(
        b, tid, B, training, seed, 0, nullptr, 0u, x, w1, b1, w2, b2,
        wf1,
        bf1, wf2, bf2, tgt, p1_ws, idx1_ws, m2_ws, p2_ws, idx2_ws,
        h1_ws, m3_ws, d3_ws, logp_ws, xs, w1s, p1, w2s, p2, d3, logits);
    if (tid == 0) lsum += -lp_t / B;
  }
  if (tid == 0) loss_part[wg] = lsum;
  grid.sync();

  // ---- phase 2: data backward -----------------------------------------
  for (int i = tid; i < N_C2K * 250; i += 256) b_w2s[i] = w2[i];
  const float sc = gl[0] / B;
  for (int bb = wg; bb < B * split; bb += nblk) {
    net_bwd_sample(bb / split, bb % split, split, tid, B, training, sc,
                   wf1, wf2, tgt, idx1_ws, m2_ws, idx2_ws, h1_ws, m3_ws,
                   logp_ws, glog_ws, gh1_ws, ga2_ws, ga1_ws,
                   b_w2s, b_glg, b_gd3, b_gh1, b_gp2, b_gd2p);
  }
  grid.sync();

  // ---- phase 3: partial weight gradients ------------------------------
  for (int t = wg; t < GW_TILES * nch; t += nblk) {
    const int tile = t % GW_TILES, ch = t / GW_TILES;
    const int b0 = ch * bchunk;
    net_gw_tile(tile, tid, b0, min(B, b0 + bchunk),
                part + (int64_t)ch * GW_ROW, x, p1_ws, p2_ws, d3_ws,
                ga1_ws, ga2_ws, gh1_ws, glog_ws);
    __syncthreads();
  }
  grid.sync();

  // ---- phase 4: combine (+ SGD), loss finalize, seed bump --------------
  const int off[9] = {OFF_W1, OFF_B1, OFF_W2, OFF_B2, OFF_WF1, OFF_BF1,
                      OFF_WF2, OFF_BF2, GW_TOTAL};
  for (int i = wg * 256 + tid; i < GW_TOTAL; i += nblk * 256) {
    const float acc = net_gw_combine_elem(i, nch, nch, nch, part);
    const int t = net_gw_tensor_of(i, off);
    const int64_t j = i - off[t];
    grd.p[t][j] = acc;
    if (do_sgd) {
      float v = acc;
      if (buf.p[t]) {
        v = mu * buf.p[t][j] + acc;
        buf.p[t][j] = v;
      }
      prm.p[t][j] -= lr * v;
    }
  }
  if (wg == 0) {
    float v = (tid < nblk) ? loss_part[tid] : 0.f;
    if (tid + 256 < nblk) v += loss_part[tid + 256];  // nblk <= 512
    smem[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (tid < s) smem[tid] += smem[tid + s];
      __syncthreads();
    }
    if (tid == 0) {
      *loss_out = smem[0];
      if (training) *seed_p = seed + SEED_INC;
    }
  }
}

namespace {

// ---- fused Net step: host layer -------------------------------------------
// the workspace's pointer vector, in NET_WS_FIELDS order
static NetWs net_ws(const std::vector<uintptr_t>& v) {
  if ((int)v.size() != NET_WS_N)
    throw std::runtime_error("net workspace: expected " +
                             std::to_string(NET_WS_N) + " pointers");
  return NetWs{(float*)v[0], (uint8_t*)v[1], (uint8_t*)v[2], (float*)v[3],
               (uint8_t*)v[4], (float*)v[5], (uint8_t*)v[6], (float*)v[7],
               (float*)v[8], (float*)v[9], (float*)v[10], (float*)v[11],
               (float*)v[12], (float*)v[13], (float*)v[14], (float*)v[15]};
}

// the 8 per-parameter pointers (conv1.w,b conv2.w,b fc1.w,b fc2.w,b)
static GwPtrs gw_ptrs(const std::vector<uintptr_t>& v, const char* what) {
  if (v.size() != 8)
    throw std::runtime_error(std::string(what) + ": expected 8 pointers");
  GwPtrs g{};
  for (int i = 0; i < 8; ++i) g.p[i] = (float*)v[i];
  return g;
}

// momentum buffers: a missing entry means "no buffer" (momentum 0)
static GwPtrs buf_ptrs(const std::vector<uintptr_t>& v) {
  GwPtrs g{};
  for (int i = 0; i < 8 && i < (int)v.size(); ++i) g.p[i] = (float*)v[i];
  return g;
}

// a per-device u32 buffer of n entries, allocated and zeroed once
// (bufs: the caller's function-local static, one slot per device)
static unsigned int* zeroed_once(unsigned int* (&bufs)[64], size_t n,
                                 hipStream_t s) {
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64) throw std::runtime_error("device index > 64");
  if (!bufs[dev]) {
    HIP_CHECK(hipMalloc(&bufs[dev], n * sizeof(unsigned int)));
    HIP_CHECK(hipMemsetAsync(bufs[dev], 0, n * sizeof(unsigned int), s));
  }
  return bufs[dev];
}

// integer environment variable (0 when unset); callers that may read
// it once per process keep the result in a function-local static
static int env_int(const char* name) {
  const char* e = std::getenv(name);
  return e ? std::atoi(e) : 0;
}

// in-launch gw fold (last-arriver epilogue in the partial kernel, no
// combine dispatch).  DTP_GW_FOLD=1 opts in; the default stays the
// two-kernel path — MEASURED NEGATIVE on both step shapes (ledger):
// the combine's dispatch latency is hidden by the stream pipeline
// (kernels enqueue back-to-back), so only its ~5 us execution is
// exposed, while the epilogue's per-block sc1-drain tail costs ~4-5 us
// across the critical path at B=128 (-5%); parity at B>=512.
static bool gw_fold_on() {
  static const bool on = env_int("DTP_GW_FOLD") != 0;
  return on;
}

// Batch chunking of the weight-gradient partial kernel, one chunk count
// per tile family (DTP_GW_NCH / _NCH1 / _NCH2 override; sweeps in
// profiles/sweeps/mfma_gw_sweep.log):
//   nch  (fc1, fc2): 16 up to B=192 (B=128: 55.5 us vs 58.3 at 24, 61.7
//        at 32), 24 above (B=512: 106.8 vs 110.3 us at 32; B=4096: 595
//        vs 634 at the old uniform 32).
//   nch1 (conv1) follows nch.  That was settled while the combine
//        folded the nch1 * 7 extension rows in a serial loop (B=128 55.2
//        us at 16 vs 58.1 at 24); the combine no longer pays per row, and
//        the re-sweep (profiles/gw_combine_numbers.md) has B=512 at 93.3
//        us with 32 vs 95.3 at 24: a lead, not yet a default.
//   nch2 (conv2), the family with the most arithmetic: 24 up to B=192
//        (B=128 55.2 us vs 56.1 at 32, 56.9 at 16), above that the most
//        rows the workspace holds (B=512 105.8 us at 32 vs 106.8 at 24).
// The fold path keeps uniform chunks (its per-column tickets assume it).
// gy is the partial kernel's gridDim.y.
struct GwPlan { int nch, nch1, nch2, bchunk, bchunk1, bchunk2, gy; };

static GwPlan gw_plan(int B) {
  static const int env_nch = env_int("DTP_GW_NCH");
  static const int env_nch1 = env_int("DTP_GW_NCH1");
  static const int env_nch2 = env_int("DTP_GW_NCH2");
  auto clamp = [B](int n) { return std::min(n, std::min(GW_MAX_CH, B)); };
  GwPlan p;
  p.nch = clamp(env_nch > 0 ? env_nch : (B <= 192 ? 16 : 24));
  if (gw_fold_on()) {
    p.nch1 = p.nch2 = p.nch;
  } else {
    p.nch1 = clamp(env_nch1 > 0 ? env_nch1 : p.nch);
    p.nch2 = clamp(env_nch2 > 0 ? env_nch2 : (B <= 192 ? 24 : 32));
  }
  p.bchunk = (B + p.nch - 1) / p.nch;
  p.bchunk1 = (B + p.nch1 - 1) / p.nch1;
  p.bchunk2 = (B + p.nch2 - 1) / p.nch2;
  p.gy = std::max(p.nch, std::max(p.nch1, p.nch2));
  return p;
}

// per-device ticket counters for the fold epilogue (GW_TILES u32,
// zeroed once; each reducer re-arms its own counter every step)
static unsigned int* gw_cnt_buf(hipStream_t s) {
  static unsigned int* bufs[64] = {};
  return zeroed_once(bufs, GW_TILES, s);
}

// which forward kernel: the re-blocked 512-thread one up to B=256, the
// 256-thread net_fwd_sample kernels (which the fwdbwd and single-launch
// kernels share) above.  kernel_micro, forward alone: 10.8 vs 16.1 us at
// B=64, 11.2-12.0 vs 16.5 at 128, 11.6 vs 17.5 at 192, 11.8 vs 17.6 at
// 256, but 156.8 vs 120.8 at 4096: at 256 VGPRs and 60 KB of LDS a CU
// holds one tiled workgroup, and three of the old ones.  Nothing was
// measured between 256 and 4096, so those batches keep what they had.
// DTP_FWD_TILED=0/1 overrides; read on every call, like DTP_BWD_TILED.
static bool fwd_tiled(int B) {
  if (const char* e = std::getenv("DTP_FWD_TILED")) return std::atoi(e) != 0;
  return B <= 256;
}

// fwd sibling split: 2 workgroups per sample when one per sample
// cannot fill the 256 CUs.  DTP_FWD_SPLIT=1 forces off, =2 forces on;
// read on every call (the microbenchmark changes it between timings).
static int fwd_split(int B) {
  const int env_v = env_int("DTP_FWD_SPLIT");
  if (B * 2 > 4096) return 1;  // loss_part/flags hold 4096 entries
  if (env_v == 1) return 1;
  if (env_v == 2) return 2;
  // 3-rep A/B (profiles/sweeps/fsplit_reps.log): +1.5% at B=64, +0.6% at
  // B=128, -2.5% at B=192 (the pair grid exceeds the CU count there
  // and the exchange round trip is pure overhead) — so the split is
  // a small-batch lever only.  Re-measured with the tiled kernel: alone it
  // is 0.5-0.9 us faster unsplit, in the step the split still wins (B=64
  // 32.91 vs 33.63 us, B=128 39.10 vs 39.91; profiles/fwd_tiled_numbers.md).
  return B <= 128 ? 2 : 1;
}

// fwd grid size (the combine kernels fold loss_part over exactly this
// many per-block partials)
static int fwd_grid(int B) {
  const int sp = fwd_split(B);
  return sp == 2 ? 2 * B : grid_for(B, 1);
}

// monotone per-process token for the split-fwd handshake: each launch
// publishes THIS value, so a stale write from a previous step's late
// sibling can never satisfy a later step's wait.  (Never returns 0,
// the flags' initial state.)
static unsigned int fwd_token() {
  static unsigned int t = 0;
  if (++t == 0) ++t;
  return t;
}

// per-device per-sample handshake flags for the split fwd (zeroed
// once; published tokens are step-unique, no re-arm needed)
static unsigned int* fwd_flags_buf(hipStream_t s) {
  static unsigned int* bufs[64] = {};
  return zeroed_once(bufs, 4096, s);
}

// Seed convention of every fused path: a training step CONSUMES the
// device seed and the kernel that ends the step (combine / fold
// epilogue) ADVANCES it, so the autograd path and the step paths can
// interleave without mask reuse.  Null = leave the seed alone.
static unsigned long long* seed_bump(bool training, uintptr_t seed_dev) {
  return training ? (unsigned long long*)seed_dev : nullptr;
}

// Forward.  loss_part mode (the step paths): per-block loss partials,
// finalized by the kernel that ends the step.  Legacy mode (the autograd
// path, net_fused_loss): a prologue dispatch zeroes the loss scalar and
// the forward accumulates into it atomically.
// how many polls sibling 0 of the tiled split forward waits for its
// sibling's token before it computes that half itself
constexpr int FWD_POLL_BOUND = 60000;

// The one place that picks the forward's kernel, block size and grid:
// tiled or net_fwd_sample kernels, split = 2 sibling workgroups per
// sample (grid 2B, blockIdx = 2b + half) or one (grid_for(B, 1)).  The
// four kernels share their leading parameters; poll_bound reaches the
// tiled split kernel only (the old one polls 60000 times).
static void launch_fwd(uintptr_t x, const GwPtrs& prm, uintptr_t tgt,
                       const NetWs& w, float* loss_part, uintptr_t seed_dev,
                       int B, bool training, bool tiled, int split,
                       int poll_bound, hipStream_t s) {
  if (tiled && (x & 15))
    throw std::invalid_argument(
        "net_fused_fwd: x must be 16-byte aligned (DTP_FWD_TILED=0 has "
        "no such requirement)");
  auto launch = [&](auto kern, int grid, int block, auto... extra) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(block), 0, s,
                       (const float*)x, prm.p[G_W1], prm.p[G_B1],
                       prm.p[G_W2], prm.p[G_B2], prm.p[G_WF1], prm.p[G_BF1],
                       prm.p[G_WF2], prm.p[G_BF2], (const int64_t*)tgt, w.p1,
                       w.idx1, w.m2, w.p2, w.idx2, w.h1, w.m3, w.d3, w.logp,
                       w.loss, loss_part,
                       (const unsigned long long*)seed_dev, B,
                       training ? 1 : 0, extra...);
  };
  if (split == 2 && tiled)
    launch(net_fused_fwd_tiled_kernel<true>, 2 * B, FT_NT, fwd_flags_buf(s),
           fwd_token(), poll_bound);
  else if (split == 2)
    launch(net_fused_fwd_split_kernel, 2 * B, 256, fwd_flags_buf(s),
           fwd_token());
  else if (tiled)
    launch(net_fused_fwd_tiled_kernel<false>, grid_for(B, 1), FT_NT,
           (unsigned int*)nullptr, 0u, 0);
  else
    launch(net_fused_fwd_kernel, grid_for(B, 1), 256);
}

void net_fused_fwd(uintptr_t x, const std::vector<uintptr_t>& prm_v,
                   uintptr_t tgt, const std::vector<uintptr_t>& ws_v,
                   bool use_loss_part, uintptr_t seed_dev, int B,
                   bool training, uintptr_t stream) {
  const NetWs w = net_ws(ws_v);
  const GwPtrs prm = gw_ptrs(prm_v, "net_fused_fwd params");
  if (!use_loss_part)
    hipLaunchKernelGGL(step_prologue_kernel, dim3(1), dim3(64), 0,
                       S(stream), (unsigned long long*)nullptr, w.loss);
  launch_fwd(x, prm, tgt, w, use_loss_part ? w.loss_part : nullptr,
             seed_dev, B, training, fwd_tiled(B), fwd_split(B),
             FWD_POLL_BOUND, S(stream));
}

// raw forward launch in loss_part mode with the kernel, the sibling split
// and the poll bound given (microbenchmarks; tests force the hand-off's
// fallback with poll_bound 0).  The loss partials are those of a
// split-`split` grid, whatever fwd_grid(B) says.
void net_fwd_raw(uintptr_t x, const std::vector<uintptr_t>& prm_v,
                 uintptr_t tgt, const std::vector<uintptr_t>& ws_v,
                 uintptr_t seed_dev, int B, bool training, bool tiled,
                 int split, int poll_bound, uintptr_t stream) {
  if (B < 1) throw std::invalid_argument("net_fwd_raw: B must be >= 1");
  if (split != 1 && split != 2)
    throw std::invalid_argument("net_fwd_raw: split must be 1 or 2");
  if (split == 2 && B * 2 > 4096)
    throw std::invalid_argument("net_fwd_raw: split 2 needs B <= 2048");
  if (poll_bound < 0)
    throw std::invalid_argument("net_fwd_raw: poll_bound must be >= 0");
  const NetWs w = net_ws(ws_v);
  launch_fwd(x, gw_ptrs(prm_v, "net_fwd_raw params"), tgt, w, w.loss_part,
             seed_dev, B, training, tiled, split, poll_bound, S(stream));
}

// sibling workgroups per sample of the data backward: enough to fill
// the 256 CUs (split=2 at B=128 — 256 workgroups, one channel half
// each — is fastest with the tiled kernel as it was with the strip
// loop; re-swept at B=64/128/4096, profiles/).
// DTP_BWD_SPLIT=1/2/4/8 overrides; read on every call, the
// microbenchmark changes it between timings.
static int bwd_split(int B) {
  int split = 0;
  if (const char* e = std::getenv("DTP_BWD_SPLIT")) split = std::atoi(e);
  if (split != 1 && split != 2 && split != 4 && split != 8) {
    split = 1;
    while (split < 8 && B * split < 256) split *= 2;
  }
  return split;
}

// which data-backward kernel: the re-blocked 512-thread one (default)
// or, with DTP_BWD_TILED=0, the 256-thread strip loop that the fwdbwd
// and single-launch kernels still share.  Read on every call, like
// DTP_BWD_SPLIT.
static bool bwd_tiled() {
  const char* e = std::getenv("DTP_BWD_TILED");
  return !(e && std::atoi(e) == 0);
}

static void launch_bwd_data(uintptr_t w2, uintptr_t wf1, uintptr_t wf2,
                            uintptr_t tgt, uintptr_t gl, const NetWs& w,
                            int B, bool training, hipStream_t s) {
  const int split = bwd_split(B);
  auto* kern = bwd_tiled() ? net_fused_bwd_tiled_kernel
                           : net_fused_bwd_kernel;
  hipLaunchKernelGGL(kern, dim3(grid_for((int64_t)B * split, 1)),
                     dim3(bwd_tiled() ? BT_NT : 256), 0, s,
                     (const float*)w2, (const float*)wf1, (const float*)wf2,
                     (const int64_t*)tgt, (const float*)gl, w.idx1, w.m2,
                     w.idx2, w.h1, w.m3, w.logp, w.glog, w.gh1, w.ga2, w.ga1,
                     B, training ? 1 : 0, split);
}

// Weight gradients, the end of every multi-dispatch step: one segmented
// partial kernel over the gw_plan chunks + one combine (no memsets, no
// atomics; any batch size), or the opt-in fold kernel.  With `sgd` the
// combine also applies the SGD+momentum update.  The kernel that ends
// the step folds the nblk_fwd per-block loss partials into loss_out
// (both null in legacy mode) and advances *seed (null = no bump).
static void launch_gw(const float* x, const NetWs& w, int B, GwPtrs gp,
                      GwPtrs pp, GwPtrs bp, float lr, float mu, bool sgd,
                      const float* loss_part, float* loss_out, int nblk_fwd,
                      unsigned long long* seed, hipStream_t s) {
  const GwPlan pl = gw_plan(B);
  if (gw_fold_on()) {
    auto* kern = !sgd ? net_gw_partial_fold_kernel<false>
                      : net_gw_partial_fold_kernel<true>;
    hipLaunchKernelGGL(kern, dim3(GW_TILES, pl.nch), dim3(256), 0, s, x, w,
                       B, pl.bchunk, gp, pp, bp, lr, mu, loss_part,
                       loss_out, nblk_fwd, seed, gw_cnt_buf(s));
    return;
  }
  hipLaunchKernelGGL(net_gw_partial_kernel, dim3(GW_TILES, pl.gy),
                     dim3(256), 0, s, x, w.p1, w.p2, w.d3, w.ga1, w.ga2,
                     w.gh1, w.glog, w.part, B, pl.bchunk, pl.bchunk1,
                     pl.bchunk2, pl.nch, pl.nch1, pl.nch2, 0);
  const dim3 grid = net_gw_combine_grid();
  if (!sgd)
    hipLaunchKernelGGL(net_gw_combine_kernel, grid, dim3(256), 0, s,
                       (const float*)w.part, gp, pl.nch, pl.nch1, pl.nch2,
                       loss_part, loss_out, nblk_fwd, seed);
  else
    hipLaunchKernelGGL(net_gw_combine_sgd_kernel, grid, dim3(256), 0, s,
                       (const float*)w.part, gp, pp, bp, pl.nch, pl.nch1,
                       pl.nch2, lr, mu, loss_part, loss_out, nblk_fwd, seed);
}

// Data backward + weight gradients.  A non-empty prm_v fuses the
// SGD+momentum update into the combine (single-GPU path: no all-reduce
// between combine and step).  Legacy mode (use_loss_part false) leaves
// the loss scalar to the forward's atomics.
void net_fused_bwd(uintptr_t x, uintptr_t w2, uintptr_t wf1, uintptr_t wf2,
                   uintptr_t tgt, uintptr_t gl,
                   const std::vector<uintptr_t>& ws_v,
                   const std::vector<uintptr_t>& grd_v,
                   const std::vector<uintptr_t>& prm_v,
                   const std::vector<uintptr_t>& buf_v, double lr, double mu,
                   int B, bool training, bool use_loss_part,
                   uintptr_t seed_dev, uintptr_t stream) {
  const NetWs w = net_ws(ws_v);
  const GwPtrs gp = gw_ptrs(grd_v, "net_fused_bwd grads");
  const bool sgd = !prm_v.empty();
  const GwPtrs pp = sgd ? gw_ptrs(prm_v, "net_fused_bwd params") : GwPtrs{};
  launch_bwd_data(w2, wf1, wf2, tgt, gl, w, B, training, S(stream));
  launch_gw((const float*)x, w, B, gp, pp, buf_ptrs(buf_v), (float)lr,
            (float)mu, sgd, use_loss_part ? w.loss_part : nullptr,
            use_loss_part ? w.loss : nullptr, fwd_grid(B),
            seed_bump(training, seed_dev), S(stream));
}

// raw data-backward launch (microbenchmarks: net_fused_bwd bundles it
// with the weight-gradient kernels)
void net_bwd_data_raw(uintptr_t w2, uintptr_t wf1, uintptr_t wf2,
                      uintptr_t tgt, uintptr_t gl,
                      const std::vector<uintptr_t>& ws_v, int B,
                      bool training, uintptr_t stream) {
  if (B < 1) throw std::invalid_argument("net_bwd_data_raw: B must be >= 1");
  launch_bwd_data(w2, wf1, wf2, tgt, gl, net_ws(ws_v), B, training,
                  S(stream));
}

#ifdef DTP_STAGE_STAMPS
// diagnostic build only: zero / read back the stage-stamp buffer as
// [STAGE_NBLK][STAGE_NSTAMP] (synchronizes the device)
void stage_stamps_clear() {
  static const std::vector<unsigned long long> z(STAGE_NBLK * STAGE_NSTAMP);
  HIP_CHECK(hipDeviceSynchronize());
  HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_stage_stamps), z.data(),
                              z.size() * sizeof(unsigned long long)));
}
std::vector<unsigned long long> stage_stamps() {
  std::vector<unsigned long long> v(STAGE_NBLK * STAGE_NSTAMP);
  HIP_CHECK(hipDeviceSynchronize());
  HIP_CHECK(hipMemcpyFromSymbol(v.data(), HIP_SYMBOL(g_stage_stamps),
                                v.size() * sizeof(unsigned long long)));
  return v;
}
#endif

// Combined fwd+bwd (one dispatch) + weight gradients: a 3-dispatch
// training step (vs 4 for fwd / bwd / partial / combine).  wts_v are
// the weights the forward reads; a non-empty prm_v also applies the
// SGD+momentum update in the combine.  Always loss_part mode, and the
// forward grid here is grid_for(B, 1) (no sibling split).
void net_fused_fwdbwd(uintptr_t x, const std::vector<uintptr_t>& wts_v,
                      uintptr_t tgt, const std::vector<uintptr_t>& ws_v,
                      const std::vector<uintptr_t>& grd_v,
                      const std::vector<uintptr_t>& prm_v,
                      const std::vector<uintptr_t>& buf_v, double lr,
                      double mu, int B, bool training, uintptr_t seed_dev,
                      uintptr_t stream) {
  const NetWs w = net_ws(ws_v);
  const GwPtrs wt = gw_ptrs(wts_v, "net_fused_fwdbwd weights");
  const GwPtrs gp = gw_ptrs(grd_v, "net_fused_fwdbwd grads");
  const bool sgd = !prm_v.empty();
  const GwPtrs pp = sgd ? gw_ptrs(prm_v, "net_fused_fwdbwd params")
                        : GwPtrs{};
  const int nblk = grid_for(B, 1);
  hipLaunchKernelGGL(net_fused_fwdbwd_kernel, dim3(nblk), dim3(256), 0,
                     S(stream),
                     NetIn{(const float*)x, (const int64_t*)tgt,
                           (const unsigned long long*)seed_dev, B,
                           training ? 1 : 0},
                     wt, w);
  launch_gw((const float*)x, w, B, gp, pp, buf_ptrs(buf_v), (float)lr,
            (float)mu, sgd, w.loss_part, w.loss, nblk,
            seed_bump(training, seed_dev), S(stream));
}

// host-only view of the chunk plan (tests, microbenchmarks)
py::dict gw_plan_py(int B) {
  if (B < 1) throw std::invalid_argument("gw_plan: B must be >= 1");
  const GwPlan p = gw_plan(B);
  py::dict d;
  d["nch"] = p.nch; d["nch1"] = p.nch1; d["nch2"] = p.nch2;
  d["bchunk"] = p.bchunk; d["bchunk1"] = p.bchunk1;
  d["bchunk2"] = p.bchunk2; d["gy"] = p.gy;
  return d;
}

// the combine clamps its row index to [0, count - 1]
static void check_gw_counts(int nch, int nch1, int nch2, const char* what) {
  for (int n : {nch, nch1, nch2})
    if (n < 1 || n > GW_MAX_CH)
      throw std::invalid_argument(std::string(what) +
                                  ": chunk counts must be in [1, 32]");
}

// raw combine launch (microbenchmarks: time the combine/sgd dispatch
// in isolation)
void net_gw_combine_raw(uintptr_t part_ws,
                        const std::vector<uintptr_t>& grd_v, int nch,
                        int nch1, int nch2,
                        uintptr_t stream) {
  const GwPtrs gp = gw_ptrs(grd_v, "net_gw_combine_raw grads");
  check_gw_counts(nch, nch1, nch2, "net_gw_combine_raw");
  hipLaunchKernelGGL(net_gw_combine_kernel,
                     net_gw_combine_grid(), dim3(256), 0,
                     S(stream), (const float*)part_ws, gp, nch, nch1,
                     nch2, nullptr, nullptr, 0, nullptr);
}

// raw combine+sgd launch (microbenchmarks)
void net_gw_combine_sgd_raw(uintptr_t part_ws,
                            const std::vector<uintptr_t>& grd_v,
                            const std::vector<uintptr_t>& prm_v,
                            const std::vector<uintptr_t>& buf_v,
                            int nch, int nch1, int nch2,
                            double lr,
                            double mu,
                            uintptr_t loss_part, uintptr_t loss_out,
                            int nblk_fwd, uintptr_t stream) {
  const GwPtrs gp = gw_ptrs(grd_v, "net_gw_combine_sgd_raw grads");
  const GwPtrs pp = gw_ptrs(prm_v, "net_gw_combine_sgd_raw params");
  check_gw_counts(nch, nch1, nch2, "net_gw_combine_sgd_raw");
  hipLaunchKernelGGL(net_gw_combine_sgd_kernel,
                     net_gw_combine_grid(), dim3(256), 0,
                     S(stream), (const float*)part_ws, gp, pp,
                     buf_ptrs(buf_v), nch,
                     nch1, nch2, (float)lr, (float)mu,
                     (const float*)loss_part, (float*)loss_out,
                     nblk_fwd, nullptr);
}

// raw tile-segment launch of the partial weight-gradient kernel
// (microbenchmarks: time [conv2 | conv1 | fc1 | fc2] separately)
void net_gw_partial_raw(uintptr_t x, uintptr_t p1_ws, uintptr_t p2_ws,
                        uintptr_t d3_ws, uintptr_t ga1_ws,
                        uintptr_t ga2_ws, uintptr_t gh1_ws,
                        uintptr_t glog_ws, uintptr_t part_ws, int B,
                        int bchunk, int bchunk1, int bchunk2,
                        int tile_base, int ntiles, int nch, int nch1,
                        int nch2, uintptr_t stream) {
  const int gy = std::max(nch, std::max(nch1, nch2));
  hipLaunchKernelGGL(net_gw_partial_kernel, dim3(ntiles, gy), dim3(256),
                     0, S(stream), (const float*)x,
                     (const float*)p1_ws, (const float*)p2_ws,
                     (const float*)d3_ws, (const float*)ga1_ws,
                     (const float*)ga2_ws, (const float*)gh1_ws,
                     (const float*)glog_ws, (float*)part_ws, B, bchunk,
                     bchunk1, bchunk2, nch, nch1, nch2, tile_base);
}


// ---- single-launch training step (cooperative) --------------------------
int net_step_max_blocks() {
  static int cached = -2;
  if (cached != -2) return cached;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { cached = 0; return 0; }
  int coop = 0;
  if (hipDeviceGetAttribute(&coop, hipDeviceAttributeCooperativeLaunch,
                            dev) != hipSuccess || !coop) {
    cached = 0;
    return 0;
  }
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(
          &per_cu, reinterpret_cast<const void*>(net_step_kernel), 256,
          0) != hipSuccess || per_cu < 1) {
    cached = 0;
    return 0;
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) {
    cached = 0;
    return 0;
  }
  int nb = per_cu * prop.multiProcessorCount;
  if (nb > 512) nb = 512;  // loss_part reduction handles <= 512
  cached = nb;
  return nb;
}

bool net_step_available() { return net_step_max_blocks() > 0; }

// Cooperative launch with the void* argument array built here.  P comes
// from the kernel's signature alone (common_type_t keeps it out of
// deduction at the arguments), so the call is checked like a direct call
// of the kernel: a missing, extra or unconvertible argument does not
// compile, and each is converted to its parameter's exact type.
template <class... P>
static void launch_coop(void (*kern)(P...), dim3 grid, dim3 block,
                        hipStream_t s, std::common_type_t<P>... a) {
  void* args[] = {&a...};
  HIP_CHECK(hipLaunchCooperativeKernel(reinterpret_cast<const void*>(kern),
                                       grid, block, args, 0, s));
}

void net_step(uintptr_t x, uintptr_t tgt, uintptr_t gl,
              const std::vector<uintptr_t>& ws_v, uintptr_t seed_dev,
              const std::vector<uintptr_t>& prm_v,
              const std::vector<uintptr_t>& grd_v,
              const std::vector<uintptr_t>& buf_v,
              double lr, double mu, bool do_sgd, int B, bool training,
              uintptr_t stream) {
  const int nblk = net_step_max_blocks();
  if (nblk < 1)
    throw std::runtime_error(
        "net_step: cooperative launch unavailable on this device");
  int split = 1;
  while (split < 8 && B * split < nblk) split *= 2;
  // its own chunking: uniform, as many of the part rows as B fills
  const int bchunk = (B + GW_MAX_CH - 1) / GW_MAX_CH;
  const int nch = (B + bchunk - 1) / bchunk;
  const NetWs w = net_ws(ws_v);
  launch_coop(net_step_kernel, dim3(nblk), dim3(256), S(stream),
              (const float*)x, (const int64_t*)tgt, (const float*)gl, w.p1,
              w.idx1, w.m2, w.p2, w.idx2, w.h1, w.m3, w.d3, w.logp, w.glog,
              w.gh1, w.ga2, w.ga1, w.part, w.loss_part, w.loss,
              (unsigned long long*)seed_dev,
              gw_ptrs(prm_v, "net_step params"),
              gw_ptrs(grd_v, "net_step grads"), buf_ptrs(buf_v), (float)lr,
              (float)mu, do_sgd ? 1 : 0, B, training ? 1 : 0, split, bchunk,
              nch);
}
}  // namespace

void register_net_fused(pybind11::module_& m) {
  m.def("net_fused_fwd", &net_fused_fwd);
  m.def("net_fwd_raw", &net_fwd_raw);
  m.def("net_fused_bwd", &net_fused_bwd);
  m.def("net_bwd_data_raw", &net_bwd_data_raw);
#ifdef DTP_STAGE_STAMPS
  m.def("stage_stamps", &stage_stamps);
  m.def("stage_stamps_clear", &stage_stamps_clear);
  m.attr("STAGE_NSTAMP") = STAGE_NSTAMP;
#endif
  m.def("net_fused_fwdbwd", &net_fused_fwdbwd);
  m.def("net_step", &net_step);
  m.def("net_step_available", &net_step_available);
  m.def("net_gw_partial_raw", &net_gw_partial_raw);
  m.def("net_gw_combine_raw", &net_gw_combine_raw);
  m.def("net_gw_combine_sgd_raw", &net_gw_combine_sgd_raw);
  m.def("gw_plan", &gw_plan_py);
  m.attr("GW_ROW") = GW_ROW;
  m.attr("GW_TOTAL") = GW_TOTAL;
  m.attr("GW_MAX_CH") = GW_MAX_CH;
  // tile counts in the order net_gw_tile walks them
  m.attr("gw_tiles") = py::make_tuple(
      py::make_tuple("conv2", T_CONV2), py::make_tuple("conv1", T_CONV1),
      py::make_tuple("fc1", T_FC1), py::make_tuple("fc2", T_FC2));
  py::list fields;
  for (const char* f : NET_WS_FIELDS) fields.append(f);
  m.attr("ws_fields") = py::tuple(fields);
}
