// nhwc_tile.h — the tiling the channels-last kernels of batchnorm_nhwc.hip
// and pool_nhwc.hip share.  A channels-last tensor is a row-major matrix of
// rows (pixels) by C channels.  In a block of BLK threads CL = 2^cl_shift
// column lanes sit side by side and own V adjacent channels each, so a row
// of the tile is one contiguous run of CT = CL*V channels; the other
// RL = BLK/CL threads are row lanes.  A thread keeps its channels for its
// whole life: per-channel constants live in registers and no index is
// divided per access.  C % V == 0 (pick_v), so a thread's V channels are
// all inside the matrix or all outside it: a ragged last column tile and
// C < CT only switch whole threads off.
#pragma once

#include "common.h"

// log2 of the column lanes of the kernels that stream whole rows: 16 (and
// 16 row lanes) from C = 128, 8 (and 32 row lanes) below, so a full-width
// tile row is 256 or 128 bytes and C = 64 still fills its tiles.  From C
// alone, so an order of summation built on the row lanes is too.
inline int nhwc_cl_shift(int64_t C) { return C >= 128 ? 4 : 3; }

struct ColTile {
  uint32_t cl, rl;  // column lane, row lane
  uint32_t c;       // the first of the thread's V channels
  bool live;        // the channels exist
};

template <int V>
__device__ __forceinline__ ColTile col_tile(uint32_t tile, int cl_shift,
                                            uint32_t C) {
  ColTile t;
  t.cl = threadIdx.x & ((1u << cl_shift) - 1u);
  t.rl = threadIdx.x >> cl_shift;
  t.c = ((tile << cl_shift) + t.cl) * V;
  t.live = t.c < C;
  return t;
}

// The sum over the row lanes of every channel of the tile, added in
// row-lane order 0, 1, ... RL-1: thread i < CT returns the sum of tile
// channel i, the others 0.  sh holds BLK*V floats.  The order is fixed by
// RL alone, so a sum built on this does not depend on V.
template <int V>
__device__ __forceinline__ float lane_combine(const float (&acc)[V],
                                              const ColTile& t, int cl_shift,
                                              float* sh) {
  const uint32_t CT = (uint32_t)V << cl_shift, RL = (uint32_t)BLK >> cl_shift;
  __syncthreads();  // sh may still be read from the previous call
#pragma unroll
  for (int j = 0; j < V; ++j) sh[t.rl * CT + t.cl * V + j] = acc[j];
  __syncthreads();
  float s = 0.f;
  if (threadIdx.x < CT) {
    s = sh[threadIdx.x];
    for (uint32_t r = 1; r < RL; ++r) s += sh[r * CT + threadIdx.x];
  }
  return s;
}

// Hands the per-channel value `mine` of thread i < CT (lane_combine's
// result, or something computed from it) to the threads that own the
// channel.  Thread i alone read sh[i] in lane_combine, so it may overwrite
// it without a barrier in between.
template <int V>
__device__ __forceinline__ void lane_broadcast(float mine, const ColTile& t,
                                               int cl_shift, float* sh,
                                               float (&out)[V]) {
  if (threadIdx.x < ((uint32_t)V << cl_shift)) sh[threadIdx.x] = mine;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < V; ++j) out[j] = sh[t.cl * V + j];
}
