// Vertical line solves for the 3-D halo stencil (gfx950): z = T^{-1} r
// along z, alone or fused into the update step of preconditioned
// conjugate gradients.  The contract is next to ZLineArgs in kernels.h.
//
// Work split.  T is the same for every column and z is never decomposed,
// so a column is a serial Thomas recurrence and the columns are the
// parallelism: one thread per interior (j, i) column, lanes along x, a
// block of 4 rows x 64 columns.  A wave's access to one plane is 64
// consecutive cells of one row, as in krylov.hip.  The factorisation was
// done on the host; a thread only multiplies, and reads inv / cp / lo / qs
// through a noalias pointer with a block-uniform index, so the table
// entries arrive by scalar loads.
//
// Data movement.  The recurrence of plane k needs plane k - 1 of the same
// thread, but its loads do not: a sweep issues the loads of kZU planes
// (up to 4 * kZU independent loads per thread in the update) before it
// runs their recurrences, which is what keeps memory busy at the low
// occupancy a large stash leaves.  The forward sweep's y_k goes to the
// thread's own LDS slots stash[k * 256 + thread] (no bank conflict, no
// barrier: nothing is shared) for k < lds_planes, and into z[k] for the
// planes above; the back sweep reads it from where it was put.
//
// Order of additions of the two inner products: a thread adds its planes
// in the order its sweep visits them, from 0, in float64; then
// krylov_block_sum for r . r, a barrier (the reduction's LDS slots are
// reused), and krylov_block_sum for r . z.  Threads past the ragged edge
// add nothing.  No atomics.

#include "kernels.h"
#include "krylov_reduce.h"

namespace {

constexpr int kZU = 4;  // planes whose loads are issued together

static_assert(kZlineBlock == kKrylovBlock &&
                  kZlineTileX * kZlineTileY == kZlineBlock &&
                  kZlineTileX == 64,
              "one wave per tile row, krylov_block_sum's block");

template <typename Acc, int MODE, bool PERIODIC>
__global__ __launch_bounds__(kZlineBlock) void zline_kernel(
    ZLineArgs a, const Acc* __restrict__ tab) {
  extern __shared__ double zline_lds[];
  Acc* stash = (Acc*)zline_lds + threadIdx.x;
  constexpr bool kUpdate = MODE == ZLINE_PCG_UPDATE;

  unsigned b = blockIdx.x;
  const unsigned tix = b % a.tiles_x;
  b /= a.tiles_x;
  const unsigned tiy = b % a.tiles_y;
  b /= a.tiles_y;
  const unsigned col = b % a.columns;
  const unsigned f = b / a.columns;
  const int nz = (int)a.nz, ls = (int)a.lds_planes;
  const long long ny = a.ny, nx = a.nx;
  const int w = a.w;
  const long long x =
      w + (long long)tix * kZlineTileX + threadIdx.x % kZlineTileX;
  const long long y =
      w + (long long)tiy * kZlineTileY + threadIdx.x / kZlineTileX;
  const long long plane = ny * nx;
  const long long first = (long long)col * nz * plane + y * nx + x;
  const Acc* inv = tab;
  const Acc* cp = tab + nz;
  const Acc* qs = tab + 2 * nz;
  const Acc* lo = tab + 3 * nz;

  double rr = 0.0, rz = 0.0;
  if (x < nx - w && y < ny - w) {
    Acc alpha = 0;
    if constexpr (kUpdate) alpha = krylov_quotient<Acc>(a.num, a.den);
    Acc* pr = (Acc*)a.r[f] + first;
    Acc* pz = (Acc*)a.z[f] + first;

    // forward sweep: (update, then) eliminate; y_k to the stash
    Acc prev = 0;
    for (int k0 = 0; k0 < nz; k0 += kZU) {
      Acc vr[kZU], vp[kZU], vq[kZU], vx[kZU];
#pragma unroll
      for (int u = 0; u < kZU; ++u) {
        const int k = k0 + u;
        if (k < nz) {
          vr[u] = pr[k * plane];
          if constexpr (kUpdate) {
            vp[u] = ((const Acc*)a.p[f] + first)[k * plane];
            vq[u] = ((const Acc*)a.q[f] + first)[k * plane];
            vx[u] = ((const Acc*)a.x[f] + first)[k * plane];
          }
        }
      }
#pragma unroll
      for (int u = 0; u < kZU; ++u) {
        const int k = k0 + u;
        if (k < nz) {
          Acc v = vr[u];
          if constexpr (kUpdate) {
            ((Acc*)a.x[f] + first)[k * plane] = vx[u] + alpha * vp[u];
            v = vr[u] - alpha * vq[u];
            pr[k * plane] = v;
            rr += (double)v * (double)v;
          }
          prev = k == 0 ? v * inv[0] : (v - lo[k] * prev) * inv[k];
          if (k < ls) {
            stash[k * kZlineBlock] = prev;
          } else {
            pz[k * plane] = prev;
          }
        }
      }
    }

    // back sweep: s_k; it is z_k unless z is periodic
    Acc next = 0, top = 0;
    for (int kt = nz - 1; kt >= 0; kt -= kZU) {
      Acc vy[kZU], vr[kZU];
#pragma unroll
      for (int u = 0; u < kZU; ++u) {
        const int k = kt - u;
        if (k >= 0) {
          vy[u] = k < ls ? stash[k * kZlineBlock] : pz[k * plane];
          if constexpr (kUpdate && !PERIODIC) vr[u] = pr[k * plane];
        }
      }
#pragma unroll
      for (int u = 0; u < kZU; ++u) {
        const int k = kt - u;
        if (k >= 0) {
          next = k == nz - 1 ? vy[u] : vy[u] - cp[k] * next;
          if (k == nz - 1) top = next;
          if constexpr (PERIODIC) {
            if (k < ls) {
              stash[k * kZlineBlock] = next;
            } else {
              pz[k * plane] = next;
            }
          } else {
            pz[k * plane] = next;
            if constexpr (kUpdate) rz += (double)vr[u] * (double)next;
          }
        }
      }
    }

    // Sherman-Morrison correction: the factor is known only now
    if constexpr (PERIODIC) {
      const Acc fac = next + lo[0] * top;
      for (int k0 = 0; k0 < nz; k0 += kZU) {
        Acc vy[kZU], vr[kZU];
#pragma unroll
        for (int u = 0; u < kZU; ++u) {
          const int k = k0 + u;
          if (k < nz) {
            vy[u] = k < ls ? stash[k * kZlineBlock] : pz[k * plane];
            if constexpr (kUpdate) vr[u] = pr[k * plane];
          }
        }
#pragma unroll
        for (int u = 0; u < kZU; ++u) {
          const int k = k0 + u;
          if (k < nz) {
            const Acc zk = vy[u] - qs[k] * fac;
            pz[k * plane] = zk;
            if constexpr (kUpdate) rz += (double)vr[u] * (double)zk;
          }
        }
      }
    }
  }

  if constexpr (kUpdate) {
    rr = krylov_block_sum(rr);
    if (threadIdx.x == 0) a.partials[blockIdx.x] = rr;
    __syncthreads();  // thread 0 has read the slots the next sum rewrites
    rz = krylov_block_sum(rz);
    if (threadIdx.x == 0) a.partials[gridDim.x + blockIdx.x] = rz;
  }
}

template <typename Acc, int MODE>
void launch_zline_t(const ZLineArgs& a, unsigned blocks, hipStream_t stream) {
  const size_t lds = (size_t)a.lds_planes * kZlineBlock * sizeof(Acc);
  dim3 grid(blocks), block(kZlineBlock);
  if (a.periodic) {
    hipLaunchKernelGGL((zline_kernel<Acc, MODE, true>), grid, block, lds,
                       stream, a, (const Acc*)a.tables);
  } else {
    hipLaunchKernelGGL((zline_kernel<Acc, MODE, false>), grid, block, lds,
                       stream, a, (const Acc*)a.tables);
  }
}

}  // namespace

hipError_t launch_zline(const ZLineArgs& a, int mode, int dt_code,
                        unsigned blocks, hipStream_t stream) {
  if (blocks == 0) return hipSuccess;
  const bool update = mode == ZLINE_PCG_UPDATE;
  if (dt_code == DT_F32 && update) {
    launch_zline_t<float, ZLINE_PCG_UPDATE>(a, blocks, stream);
  } else if (dt_code == DT_F32) {
    launch_zline_t<float, ZLINE_SOLVE>(a, blocks, stream);
  } else if (dt_code == DT_F64 && update) {
    launch_zline_t<double, ZLINE_PCG_UPDATE>(a, blocks, stream);
  } else if (dt_code == DT_F64) {
    launch_zline_t<double, ZLINE_SOLVE>(a, blocks, stream);
  }  // anything else is rejected by the host-side check in bridge.cpp
  return hipGetLastError();
}
