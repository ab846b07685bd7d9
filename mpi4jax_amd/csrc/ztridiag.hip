// Per-column tridiagonal solves along z (gfx950): one system per interior
// (j, i) with bands that vary by cell, factorised once (FACTOR + SOLVE) or
// inside the solve's own launch (SOLVE_BANDS).  The contract is next to
// ZTridiagArgs in kernels.h.
//
// Work split.  As in zline.hip a column is a serial Thomas recurrence and
// the columns are the parallelism: one thread per interior (j, i), lanes
// along x, a block of 4 rows x 64 cells, so a wave's access to a plane is
// 64 consecutive cells of one row.  Unlike there the factors are fields,
// not tables: every plane of a march costs a load of lo / inv (forward) and
// cp (back) per thread, and memory traffic is the whole cost.
//
// Right-hand sides per thread.  A thread carries R = 1, 2 or 4 consecutive
// entries of the flattened (field, batch column) list through one march, so
// the factor loads (on the fused path the band loads, the float64 pivot and
// its division) are paid once per R recurrences: 2 + 3 / R field-sized
// streams per right-hand side instead of 5.  The recurrences of the R
// entries are independent and written once, in `forward_row` / the back
// loop, so what one entry computes does not depend on R; slots past a
// ragged last group are neither loaded, computed nor stored.
//
// LDS.  y_k of the R entries (and cp_k on the fused path) go to the
// thread's own slots stash[(k * slots + s) * 256 + thread] for
// k < lds_planes: no barrier and no bank conflict, because nothing is
// shared.  The planes above go through the output array (y) and through
// the solver's workspace (the fused cp).
//
// Loads in flight.  A 64 KB stash leaves about two blocks per CU, so a
// sweep issues every load of kTU = 4 planes (all right-hand sides and all
// bands of those planes) before it runs their recurrences.  Four planes
// give 12 (R = 1) to 28 (fused, R = 4) independent loads per thread, at
// most 56 VGPRs in float64, which two waves per SIMD hold without
// spilling; eight planes would double that for R = 4 and start to cost
// occupancy at small stashes.  One value for every R keeps the sweeps of
// one right-hand side identical across R.
//
// The factor kernel runs the same float64 recurrence (`pivot_row`) as the
// fused path and rounds once, so both produce the same factors bit for bit.
// Its status is one vector store of two doubles per block; no atomics.

#include "kernels.h"

#include <limits>

namespace {

constexpr int kTU = 4;  // planes whose loads are issued together

static_assert(kZlineTileX * kZlineTileY == kZlineBlock && kZlineTileX == 64,
              "one wave per tile row");

// Row k of the float64 factorisation: the pivot from the row's bands and
// the row below's cp, then inv = 1 / pivot and cp = u inv (returned in
// `cp`).  Row 0 does not read l.
__device__ __forceinline__ double pivot_row(int k, double l, double d,
                                            double u, double& cp,
                                            double& pivot) {
  pivot = k == 0 ? d : d - l * cp;
  const double inv = 1.0 / pivot;
  cp = u * inv;
  return inv;
}

// y_k from r_k and y_{k-1}
template <typename Acc>
__device__ __forceinline__ Acc forward_row(int k, Acc r, Acc lo, Acc inv,
                                           Acc prev) {
  return k == 0 ? r * inv : (r - lo * prev) * inv;
}

struct Tile {
  long long cell, plane;  // offset of (y, x) inside a plane; ny * nx
  unsigned group;         // what is left of the block index
  bool inside;
};

__device__ __forceinline__ Tile decode_tile(const ZTridiagArgs& a) {
  unsigned b = blockIdx.x;
  const unsigned tix = b % a.tiles_x;
  b /= a.tiles_x;
  const unsigned tiy = b % a.tiles_y;
  const long long x =
      a.w + (long long)tix * kZlineTileX + threadIdx.x % kZlineTileX;
  const long long y =
      a.w + (long long)tiy * kZlineTileY + threadIdx.x / kZlineTileX;
  return Tile{y * a.nx + x, a.ny * a.nx, b / a.tiles_y,
              x < a.nx - a.w && y < a.ny - a.w};
}

template <typename Acc, typename Band>
__global__ __launch_bounds__(kZlineBlock) void ztridiag_factor_kernel(
    ZTridiagArgs a) {
  __shared__ double red[2 * kZlineBlock / 64];
  const Tile t = decode_tile(a);
  const int nz = (int)a.nz;
  // the smallest pivot up to and including the column's first bad one
  double low = std::numeric_limits<double>::infinity(), low_k = 0.0;
  if (t.inside) {
    const Band* pl = (const Band*)a.lower + t.cell;
    const Band* pd = (const Band*)a.diag + t.cell;
    const Band* pu = (const Band*)a.upper + t.cell;
    Acc* finv = (Acc*)a.factors + t.cell;
    Acc* fcp = finv + nz * t.plane;
    Acc* flo = fcp + nz * t.plane;
    double cp = 0.0;
    bool alive = true;
    for (int k0 = 0; k0 < nz; k0 += kTU) {
      double bl[kTU], bd[kTU], bu[kTU];
#pragma unroll
      for (int u = 0; u < kTU; ++u) {
        const int k = k0 + u;
        if (k < nz) {
          bl[u] = (double)pl[k * t.plane];
          bd[u] = (double)pd[k * t.plane];
          bu[u] = (double)pu[k * t.plane];
        }
      }
#pragma unroll
      for (int u = 0; u < kTU; ++u) {
        const int k = k0 + u;
        if (k < nz) {
          double pivot;
          const double inv = pivot_row(k, bl[u], bd[u], bu[u], cp, pivot);
          finv[k * t.plane] = (Acc)inv;
          fcp[k * t.plane] = (Acc)cp;
          flo[k * t.plane] = (Acc)bl[u];
          const double m = __builtin_isfinite(pivot)
                               ? pivot
                               : -std::numeric_limits<double>::infinity();
          if (alive && m < low) {
            low = m;
            low_k = (double)k;
          }
          alive = alive && m > 0.0;
        }
      }
    }
  }
  // block minimum of (low, low_k): lanes, then the four waves
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const double o = __shfl_xor(low, d, 64), ok = __shfl_xor(low_k, d, 64);
    if (o < low || (o == low && ok < low_k)) {
      low = o;
      low_k = ok;
    }
  }
  if (threadIdx.x % 64 == 0) {
    red[2 * (threadIdx.x / 64)] = low;
    red[2 * (threadIdx.x / 64) + 1] = low_k;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int v = 1; v < kZlineBlock / 64; ++v) {
      if (red[2 * v] < low || (red[2 * v] == low && red[2 * v + 1] < low_k)) {
        low = red[2 * v];
        low_k = red[2 * v + 1];
      }
    }
    a.status[2 * blockIdx.x] = low;
    a.status[2 * blockIdx.x + 1] = low_k;
  }
}

template <typename Acc, typename Band, int R, bool FUSED>
__global__ __launch_bounds__(kZlineBlock) void ztridiag_solve_kernel(
    ZTridiagArgs a) {
  extern __shared__ double ztridiag_lds[];
  constexpr int kSlots = R + (FUSED ? 1 : 0);
  constexpr int kRow = kSlots * kZlineBlock;  // stash values per plane
  Acc* stash = (Acc*)ztridiag_lds + threadIdx.x;
  const Tile t = decode_tile(a);
  if (!t.inside) return;  // no barrier below
  const int nz = (int)a.nz, ls = (int)a.lds_planes;
  const long long plane = t.plane;

  // the group's right-hand sides; nr < R in a ragged last group
  const unsigned s0 = t.group * R;
  const int nr = (int)(a.nrhs - s0 < (unsigned)R ? a.nrhs - s0 : R);
  const Acc* pr[R];
  Acc* px[R];
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const unsigned s = s0 + (j < nr ? j : 0);
    const long long off = (long long)(s % a.batch) * nz * plane + t.cell;
    pr[j] = (const Acc*)a.r[s / a.batch] + off;
    px[j] = (Acc*)a.x[s / a.batch] + off;
  }
  const Acc* finv = (const Acc*)a.factors + t.cell;
  const Acc* fcp = finv + nz * plane;
  const Acc* flo = fcp + nz * plane;
  const Band* pl = (const Band*)a.lower + t.cell;
  const Band* pd = (const Band*)a.diag + t.cell;
  const Band* pu = (const Band*)a.upper + t.cell;
  // fused: cp of plane k >= ls at pw[(k - ls) * plane]
  Acc* pw = (Acc*)a.work + (long long)t.group * (nz - ls) * plane + t.cell;

  // forward sweep: y_k to the stash, or to x[k] above it
  Acc prev[R];
#pragma unroll
  for (int j = 0; j < R; ++j) prev[j] = 0;
  double cp64 = 0.0;
  for (int k0 = 0; k0 < nz; k0 += kTU) {
    Acc vr[kTU][R], vi[kTU], vl[kTU];
    double bl[kTU], bd[kTU], bu[kTU];
#pragma unroll
    for (int u = 0; u < kTU; ++u) {
      const int k = k0 + u;
      if (k < nz) {
        if constexpr (FUSED) {
          bl[u] = (double)pl[k * plane];
          bd[u] = (double)pd[k * plane];
          bu[u] = (double)pu[k * plane];
        } else {
          vi[u] = finv[k * plane];
          vl[u] = flo[k * plane];
        }
#pragma unroll
        for (int j = 0; j < R; ++j) {
          if (j < nr) vr[u][j] = pr[j][k * plane];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kTU; ++u) {
      const int k = k0 + u;
      if (k < nz) {
        Acc inv, lo;
        if constexpr (FUSED) {
          double pivot;
          inv = (Acc)pivot_row(k, bl[u], bd[u], bu[u], cp64, pivot);
          lo = (Acc)bl[u];
          if (k < ls) {
            stash[k * kRow + R * kZlineBlock] = (Acc)cp64;
          } else {
            pw[(k - ls) * plane] = (Acc)cp64;
          }
        } else {
          inv = vi[u];
          lo = vl[u];
        }
#pragma unroll
        for (int j = 0; j < R; ++j) {
          if (j < nr) {
            prev[j] = forward_row(k, vr[u][j], lo, inv, prev[j]);
            if (k < ls) {
              stash[k * kRow + j * kZlineBlock] = prev[j];
            } else {
              px[j][k * plane] = prev[j];
            }
          }
        }
      }
    }
  }

  // back sweep: x_k = y_k - cp_k x_{k+1}
  Acc next[R];
#pragma unroll
  for (int j = 0; j < R; ++j) next[j] = 0;
  for (int kt = nz - 1; kt >= 0; kt -= kTU) {
    Acc vy[kTU][R], vc[kTU];
#pragma unroll
    for (int u = 0; u < kTU; ++u) {
      const int k = kt - u;
      if (k >= 0) {
        if constexpr (FUSED) {
          vc[u] = k < ls ? stash[k * kRow + R * kZlineBlock]
                         : pw[(k - ls) * plane];
        } else {
          vc[u] = fcp[k * plane];
        }
#pragma unroll
        for (int j = 0; j < R; ++j) {
          if (j < nr) {
            vy[u][j] =
                k < ls ? stash[k * kRow + j * kZlineBlock] : px[j][k * plane];
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kTU; ++u) {
      const int k = kt - u;
      if (k >= 0) {
#pragma unroll
        for (int j = 0; j < R; ++j) {
          if (j < nr) {
            next[j] = k == nz - 1 ? vy[u][j] : vy[u][j] - vc[u] * next[j];
            px[j][k * plane] = next[j];
          }
        }
      }
    }
  }
}

template <typename Acc, typename Band, int R, bool FUSED>
void launch_solve_r(const ZTridiagArgs& a, unsigned blocks,
                    hipStream_t stream) {
  const size_t lds = (size_t)a.lds_planes * (R + (FUSED ? 1 : 0)) *
                     kZlineBlock * sizeof(Acc);
  hipLaunchKernelGGL((ztridiag_solve_kernel<Acc, Band, R, FUSED>),
                     dim3(blocks), dim3(kZlineBlock), lds, stream, a);
}

template <typename Acc, typename Band, bool FUSED>
void launch_solve_t(const ZTridiagArgs& a, int rhs_per_thread,
                    unsigned blocks, hipStream_t stream) {
  if (rhs_per_thread == 1) {
    launch_solve_r<Acc, Band, 1, FUSED>(a, blocks, stream);
  } else if (rhs_per_thread == 2) {
    launch_solve_r<Acc, Band, 2, FUSED>(a, blocks, stream);
  } else if (rhs_per_thread == 4) {
    launch_solve_r<Acc, Band, 4, FUSED>(a, blocks, stream);
  }
}

template <typename Acc, typename Band>
void launch_op(const ZTridiagArgs& a, int op, int rhs_per_thread,
               unsigned blocks, hipStream_t stream) {
  if (op == ZTRIDIAG_FACTOR) {
    hipLaunchKernelGGL((ztridiag_factor_kernel<Acc, Band>), dim3(blocks),
                       dim3(kZlineBlock), 0, stream, a);
  } else if (op == ZTRIDIAG_SOLVE_BANDS) {
    launch_solve_t<Acc, Band, true>(a, rhs_per_thread, blocks, stream);
  }
}

}  // namespace

hipError_t launch_ztridiag(const ZTridiagArgs& a, int op, int dt_code,
                           int band_code, int rhs_per_thread,
                           unsigned blocks, hipStream_t stream) {
  if (blocks == 0) return hipSuccess;
  const bool f64 = dt_code == DT_F64, b64 = band_code == DT_F64;
  if ((dt_code != DT_F32 && !f64) ||
      (op != ZTRIDIAG_SOLVE && band_code != DT_F32 && !b64)) {
    return hipGetLastError();  // rejected by the host-side check
  }
  if (op == ZTRIDIAG_SOLVE) {  // reads no band
    if (f64) {
      launch_solve_t<double, double, false>(a, rhs_per_thread, blocks, stream);
    } else {
      launch_solve_t<float, float, false>(a, rhs_per_thread, blocks, stream);
    }
  } else if (f64 && b64) {
    launch_op<double, double>(a, op, rhs_per_thread, blocks, stream);
  } else if (f64) {
    launch_op<double, float>(a, op, rhs_per_thread, blocks, stream);
  } else if (b64) {
    launch_op<float, double>(a, op, rhs_per_thread, blocks, stream);
  } else {
    launch_op<float, float>(a, op, rhs_per_thread, blocks, stream);
  }
  return hipGetLastError();
}
