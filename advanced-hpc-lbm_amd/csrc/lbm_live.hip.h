// lbm_live.hip.h -- the one kernel behind lbm_set_obstacles: a slab's obstacle bytes replaced from the
// new map, the cells that turn from blocked to fluid refilled with the rest equilibrium, and counted.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lbm_kernels.hip.h"

namespace lbm {

// Blocks of one lbm_swap_blocked launch at the most: a block walks the slab's cells with the stride of the grid, so the
// count comes back as at most this many integers whatever the lattice.
constexpr int kSwapBlocksMax = 4096;

// obst: the slab's rows of the new map, int[ncell] (row-major, nx per row).  blocked: the slab's bytes (pitch per row), read
// (the old map) and rewritten (the new one) cell by cell, each cell by one thread.  refill != 0: a cell blocked before and
// fluid now gets (w0, w1 x 4, w2 x 4) in the nine planes of lat, the lattice that holds the current state.  counts[block] =
// the cells this block refilled: a wave reduction by shuffles, the waves' sums through LDS, ONE plain store per block --
// an integer sum, so no order to fix; no atomics.  Every other cell's populations are not touched.
__global__ __launch_bounds__(kBlock) void lbm_swap_blocked(const int* obst, uint8_t* blocked, float* lat, long plane, int pitch,
                                                           int nx, long ncell, int refill, float w0, float w1, float w2,
                                                           int* counts) {
  __shared__ int red[kBlock / 64];
  int n = 0;
  const long stride = (long)gridDim.x * kBlock;
  for (long c = (long)blockIdx.x * kBlock + threadIdx.x; c < ncell; c += stride) {
    const long y = c / nx; const int x = (int)(c - y * nx);
    const long o = y * pitch + x;
    const uint8_t was = blocked[o], now = obst[c] ? 1 : 0;
    if (was != now) blocked[o] = now;
    if (refill && was && !now) {
      lat[o] = w0;
#pragma unroll
      for (int k = 1; k < 5; ++k) lat[k * plane + o] = w1;
#pragma unroll
      for (int k = 5; k < 9; ++k) lat[k * plane + o] = w2;
      ++n;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) red[wave] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    int r = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) r += red[w];
    counts[blockIdx.x] = r;
  }
}

}  // namespace lbm
