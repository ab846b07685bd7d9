// The block reduction of every float64 inner product (krylov.hip and the
// DOT epilogue of stencil.hip).  No atomics, one fixed order:
//   1. a thread has added its own terms in a fixed order (the callers say
//      which);
//   2. a wave adds its 64 lanes by the shuffle tree below: lane l takes
//      lane l + 32, then l + 16, ..., then l + 1, so lane 0 ends with the
//      wave's sum;
//   3. lane 0 of wave k stores that sum into LDS slot k, and thread 0 adds
//      the slots from 0 in wave order.
// Thread 0 returns the block's sum; what the other threads return is not
// meaningful.  Every thread of the block must call it (it synchronises).
#pragma once

#include <hip/hip_runtime.h>

constexpr int kKrylovBlock = 256;  // threads of every caller's block
constexpr int kKrylovWaves = kKrylovBlock / 64;

__device__ inline double krylov_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

__device__ inline double krylov_block_sum(double v) {
  __shared__ double wave_sums[kKrylovWaves];
  v = krylov_wave_sum(v);
  if (threadIdx.x % 64 == 0) wave_sums[threadIdx.x / 64] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < kKrylovWaves; ++k) s += wave_sums[k];
  }
  return s;
}
