// Vertical line solves by parallel cyclic reduction (gfx950): z = T^{-1} r
// along z, alone or fused into the update step of preconditioned conjugate
// gradients, for tall columns on small planes.  The contract is next to
// ZLinePcrArgs in kernels.h.
//
// Work split.  zline.hip gives a column to one thread, so a 16 x 16 plane
// is 256 threads that each wait on 2 nz dependent steps.  Here the planes
// of a column are the parallelism as well: a block owns C consecutive
// cells of one row, all nz planes of them, and its 256 threads are C lanes
// along x times P = 256 / C planes in flight.  T is the same for every
// column, so the host has reduced it already (the tables of kernels.h) and
// a level of the reduction is two multiply-adds per value:
// ceil(log2 nz) levels, each one pass of the block over its nz x C values.
//
// Data movement.  Every plane of the tile is loaded once, kZU planes'
// loads in flight per thread before the first LDS write, into buffer 0 of
// two [k][lane] buffers.  A level reads planes k, k - s and k + s of one
// buffer and writes plane k of the other; one barrier ends it.  Threads
// t, t + 1 hold lanes lane, lane + 1 of a plane and thread t + C lane 0 of
// the next plane, so a wave reads 64 consecutive values of each of the
// three planes: no bank conflict at any C.  After the last level
// z_k = v_k inv_k goes straight to global memory; under periodic z s_k
// goes back to LDS, and after one more barrier every thread reads s_0 and
// s_{nz-1} of its lane for the Sherman-Morrison correction.
//
// C is a kernel argument, not a template parameter: all tile widths run
// the same instructions on a cell, so the result does not depend on C bit
// for bit.  The table entries (2 ceil(log2 nz) + 2 rows of nz) are read
// per thread through a noalias pointer; k is uniform over a wave only at
// C = 64, so these are vector loads that hit in L1 after the first wave.
// LDS has no room for them next to the buffers at the heights this kernel
// is for.  No other way of reading them has been timed.
//
// Order of additions of the two inner products: a thread adds its planes
// in ascending k, in float64; then krylov_block_sum for r . r, a barrier
// (the reduction's LDS slots are reused), and krylov_block_sum for r . z.
// Threads past the ragged edge load, store and add nothing, but take
// every barrier.  No atomics.

#include "kernels.h"
#include "krylov_reduce.h"

namespace {

constexpr int kZU = 4;  // planes whose global loads are issued together

static_assert(kZlineBlock == kKrylovBlock, "krylov_block_sum's block");

template <typename Acc, bool UPDATE, bool PERIODIC>
__global__ __launch_bounds__(kZlineBlock) void zline_pcr_kernel(
    ZLinePcrArgs a, const Acc* __restrict__ tab) {
  extern __shared__ double zline_pcr_lds[];
  const int nz = (int)a.nz, levels = (int)a.levels, lc = (int)a.cols_log2;
  const int lane = threadIdx.x & ((1 << lc) - 1);
  const int zl = threadIdx.x >> lc, step = kZlineBlock >> lc;
  Acc* src = (Acc*)zline_pcr_lds + lane;  // [k << lc]: plane k, this lane
  Acc* dst = src + ((size_t)nz << lc);

  unsigned b = blockIdx.x;
  const unsigned tix = b % a.tiles_x;
  b /= a.tiles_x;
  const unsigned row = b % a.rows;
  b /= a.rows;
  const unsigned col = b % a.columns;
  const unsigned f = b / a.columns;
  const long long nx = a.nx, plane = a.ny * a.nx;
  const int w = a.w;
  const long long x = w + ((long long)tix << lc) + lane;
  const long long y = w + (long long)row;
  const long long first = (long long)col * nz * plane + y * nx + x;
  const bool live = x < nx - w;
  Acc* pr = (Acc*)a.r[f] + first;
  Acc* pz = (Acc*)a.z[f] + first;

  // load (update first): every plane of the tile into buffer 0
  double rr = 0.0, rz = 0.0;
  if (live) {
    Acc alpha = 0;
    if constexpr (UPDATE) alpha = krylov_quotient<Acc>(a.num, a.den);
    for (int k0 = zl; k0 < nz; k0 += kZU * step) {
      Acc vr[kZU], vp[kZU], vq[kZU], vx[kZU];
#pragma unroll
      for (int u = 0; u < kZU; ++u) {
        const int k = k0 + u * step;
        if (k < nz) {
          vr[u] = pr[k * plane];
          if constexpr (UPDATE) {
            vp[u] = ((const Acc*)a.p[f] + first)[k * plane];
            vq[u] = ((const Acc*)a.q[f] + first)[k * plane];
            vx[u] = ((const Acc*)a.x[f] + first)[k * plane];
          }
        }
      }
#pragma unroll
      for (int u = 0; u < kZU; ++u) {
        const int k = k0 + u * step;
        if (k < nz) {
          Acc v = vr[u];
          if constexpr (UPDATE) {
            ((Acc*)a.x[f] + first)[k * plane] = vx[u] + alpha * vp[u];
            v = vr[u] - alpha * vq[u];
            pr[k * plane] = v;
            rr += (double)v * (double)v;
          }
          src[k << lc] = v;
        }
      }
    }
  }
  __syncthreads();

  // the levels: v'_k = v_k + alpha_k v_{k-s} + gamma_k v_{k+s}
  for (int l = 0; l < levels; ++l) {
    if (live) {
      const int s = 1 << l;
      const Acc* al = tab + (size_t)l * nz;
      const Acc* ga = tab + (size_t)(levels + l) * nz;
#pragma unroll 4
      for (int k = zl; k < nz; k += step) {
        Acc v = src[k << lc];
        if (k >= s) v += al[k] * src[(k - s) << lc];
        if (k + s < nz) v += ga[k] * src[(k + s) << lc];
        dst[k << lc] = v;
      }
    }
    __syncthreads();
    Acc* t = src;
    src = dst;
    dst = t;
  }

  const Acc* inv = tab + (size_t)2 * levels * nz;
  if constexpr (PERIODIC) {
    if (live) {
      for (int k = zl; k < nz; k += step) dst[k << lc] = src[k << lc] * inv[k];
    }
    __syncthreads();
    src = dst;
  }

  // store: z_k, and the update's r . z on the stored r
  if (live) {
    const Acc* qs = inv + nz;
    Acc fac = 0;
    if constexpr (PERIODIC) fac = src[0] + tab[0] * src[(nz - 1) << lc];
    for (int k0 = zl; k0 < nz; k0 += kZU * step) {
      Acc vr[kZU];
      if constexpr (UPDATE) {
#pragma unroll
        for (int u = 0; u < kZU; ++u) {
          const int k = k0 + u * step;
          if (k < nz) vr[u] = pr[k * plane];
        }
      }
#pragma unroll
      for (int u = 0; u < kZU; ++u) {
        const int k = k0 + u * step;
        if (k < nz) {
          Acc zk;
          if constexpr (PERIODIC) {
            zk = src[k << lc] - qs[k] * fac;
          } else {
            zk = src[k << lc] * inv[k];
          }
          pz[k * plane] = zk;
          if constexpr (UPDATE) rz += (double)vr[u] * (double)zk;
        }
      }
    }
  }

  if constexpr (UPDATE) {
    rr = krylov_block_sum(rr);
    if (threadIdx.x == 0) a.partials[blockIdx.x] = rr;
    __syncthreads();  // thread 0 has read the slots the next sum rewrites
    rz = krylov_block_sum(rz);
    if (threadIdx.x == 0) a.partials[gridDim.x + blockIdx.x] = rz;
  }
}

template <typename Acc, bool UPDATE>
void launch_zline_pcr_t(const ZLinePcrArgs& a, unsigned blocks,
                        hipStream_t stream) {
  const size_t lds = ((size_t)2 * a.nz << a.cols_log2) * sizeof(Acc);
  dim3 grid(blocks), block(kZlineBlock);
  if (a.periodic) {
    hipLaunchKernelGGL((zline_pcr_kernel<Acc, UPDATE, true>), grid, block,
                       lds, stream, a, (const Acc*)a.tables);
  } else {
    hipLaunchKernelGGL((zline_pcr_kernel<Acc, UPDATE, false>), grid, block,
                       lds, stream, a, (const Acc*)a.tables);
  }
}

}  // namespace

hipError_t launch_zline_pcr(const ZLinePcrArgs& a, int mode, int dt_code,
                            unsigned blocks, hipStream_t stream) {
  if (blocks == 0) return hipSuccess;
  const bool update = mode == ZLINE_PCG_UPDATE;
  if (dt_code == DT_F32 && update) {
    launch_zline_pcr_t<float, true>(a, blocks, stream);
  } else if (dt_code == DT_F32) {
    launch_zline_pcr_t<float, false>(a, blocks, stream);
  } else if (dt_code == DT_F64 && update) {
    launch_zline_pcr_t<double, true>(a, blocks, stream);
  } else if (dt_code == DT_F64) {
    launch_zline_pcr_t<double, false>(a, blocks, stream);
  }  // anything else is rejected by the host-side check in bridge.cpp
  return hipGetLastError();
}
