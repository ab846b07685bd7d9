// 3-D halo stencil kernel (gfx950) of parallel/stencil3d.HaloStencil3D: a
// 2.5-D march along z.  The contract is next to HaloStencil3dArgs in
// kernels.h.
//
// A 256-thread workgroup owns one 32 x 64 tile (the tile grid of
// stencil.hip) of one column and marches over the output planes
// [z0, z1) of its chunk.  Wave k of the four owns rows k, k + 4, ... of the
// tile and a lane one column, so a thread has 8 cells of every plane.
//
// Only ONE input plane, with its w-cell apron and converted to the
// accumulate type, is resident in LDS for the tap loop; a second LDS buffer
// takes the next plane, so a plane costs one barrier and a wave that is
// through with plane s fills plane s + 1 while the others still sum.  An
// input plane is read from memory once per block.  The fills are those of
// stencil.hip (register-staged straight fill for tiles wholly inside the
// interior, the 3 x 3 region table otherwise); a plane's halo geometry does
// not depend on z.
//
// A thread keeps (2 RZ + 1) x 8 partial outputs in registers, RZ a template
// parameter.  With input plane s resident it adds K_t * v[s] into the
// accumulators of output plane s - dz_t; slot j of acc[][] belongs to
// dz = j - RZ, so every index is a compile-time constant.  The taps of one
// dz are contiguous in the tap list (tap_begin) and go in list order.  The
// march goes upward, so an output plane receives dz = -RZ first and
// dz = +RZ last: the order of additions per output is the order of the tap
// list.  After plane s the output plane s - RZ is complete: slot 2 RZ is
// stored, the slots shift up by one and slot 0 restarts from 0.  The shift
// costs 2 RZ x 8 register moves per plane; unrolling the march by
// 2 RZ + 1 instead would save them at three to five times the code.
//
// Transposed mode: the LDS plane holds gout (zero outside the interior),
// the in-plane offsets arrive negated, and the march goes DOWNWARD
// (output plane s + dz_t), which again gives every output its terms in
// tap-list order.
//
// z boundary: a source plane outside [0, nz) is wrapped (periodic) or, under
// the zero boundary, neither filled nor summed: its taps add nothing.
//
// DOT: when output plane k retires, the thread adds
// double(in[k] at the cell, re-read from memory) * double(output as
// stored) for its 8 rows in order, planes in march order, from 0; after
// the march one krylov_block_sum and one store to partials[blockIdx.x].

#include "halo_types.h"
#include "kernels.h"
#include "krylov_reduce.h"
#include "stencil_cells.h"

#include <cstdint>

namespace {

constexpr int kS3Block = kStencilBlock;
constexpr int kS3TX = kStencilTileX;
constexpr int kS3TY = kStencilTileY;
constexpr int kS3Waves = kS3Block / kS3TX;
constexpr int kS3Rows = kS3TY / kS3Waves;  // cells per thread and plane
constexpr int kS3FillIts =
    (kS3TY + 2 * kStencilMaxWidth + kS3Waves - 1) / kS3Waves;

static_assert(kS3Block == kKrylovBlock,
              "the dot epilogue reduces over a block of the Krylov size");
static_assert(2 * kStencilMaxWidth <= kS3TX,
              "the apron columns are filled by one partial pass");

// One input plane `in` (plane index `pl` of the slot layout) into the LDS
// buffer `tile`: rows fy0 .. of (kS3TY + 2w) x (kS3TX + 2w) cells.
template <typename T, typename Acc, int MODE>
__device__ inline void stencil3d_fill(const HaloStencil3dArgs& a, Acc* tile,
                                      const T* in, unsigned pl, bool fast,
                                      long long fy0, long long fx0, int lane,
                                      int wrow) {
  const int w = a.w;
  const int S = kS3TX + 2 * w;
  const int rows = kS3TY + 2 * w;
  const long long ny = a.ny, nx = a.nx;
  if (fast) {
    // all of a wave's global loads are issued before the first LDS store
    T main[kS3FillIts], side[kS3FillIts];
    const T* src = in + ((fy0 + wrow) * nx + fx0 + lane);
#pragma unroll
    for (int it = 0; it < kS3FillIts; ++it) {
      if (wrow + it * kS3Waves < rows) {
        const T* p = src + (long long)it * kS3Waves * nx;
        main[it] = p[0];
        if (lane < 2 * w) side[it] = p[kS3TX];
      }
    }
#pragma unroll
    for (int it = 0; it < kS3FillIts; ++it) {
      const int r = wrow + it * kS3Waves;
      if (r < rows) {
        tile[r * S + lane] = adj_load<T, Acc>(&main[it]);
        if (lane < 2 * w) {
          tile[r * S + kS3TX + lane] = adj_load<T, Acc>(&side[it]);
        }
      }
    }
    return;
  }
  for (int r = wrow; r < rows; r += kS3Waves) {
    const long long y = fy0 + r;
    for (int c = lane; c < S; c += kS3TX) {
      tile[r * S + c] =
          stencil_slow_cell<T, Acc, MODE>(a, in, pl, y, fx0 + c, w, ny, nx);
    }
  }
}

template <typename T, typename Acc, int RZ, int MODE, bool DOT>
__global__ __launch_bounds__(kS3Block) void halo_stencil3d_kernel(
    HaloStencil3dArgs a) {
  constexpr int N = 2 * RZ + 1;
  constexpr int DIR = MODE == 0 ? 1 : -1;  // the march's direction in z
  static_assert(!DOT || MODE == 0, "the dot epilogue belongs to apply");
  extern __shared__ __align__(16) unsigned char stencil3d_lds[];
  const int w = a.w;
  const int S = kS3TX + 2 * w;     // LDS row stride
  const int rows = kS3TY + 2 * w;  // LDS rows
  Acc* const buf0 = (Acc*)stencil3d_lds;
  Acc* const buf1 = buf0 + rows * S;
  unsigned b = blockIdx.x;
  const unsigned tix = b % a.tiles_x;
  b /= a.tiles_x;
  const unsigned tiy = b % a.tiles_y;
  b /= a.tiles_y;
  const unsigned ch = b % a.chunks;
  b /= a.chunks;
  const unsigned col = b % a.columns;
  const unsigned f = b / a.columns;
  const int nz = (int)a.nz;
  const int z0 = (int)(ch * a.zc);
  const int z1 = z0 + (int)a.zc < nz ? z0 + (int)a.zc : nz;
  const long long ny = a.ny, nx = a.nx;
  const long long plane = ny * nx;
  const unsigned lev0 = col * a.nz;          // level of plane 0 of the column
  const unsigned pl0 = f * a.levels + lev0;  // its plane in the slot layout
  const T* in = (const T*)a.in[f] + (long long)lev0 * plane;
  T* out = (T*)a.out[f] + (long long)lev0 * plane;
  // the output domain: the interior (apply) or the full array (transposed)
  const int org = MODE == 0 ? w : 0;
  const long long oy0 = org + (long long)tiy * kS3TY;
  const long long ox0 = org + (long long)tix * kS3TX;
  const long long fy0 = oy0 - w, fx0 = ox0 - w;  // first cell of the tile
  const int lane = threadIdx.x % kS3TX;
  const int wrow = threadIdx.x / kS3TX;
  const long long ylim = MODE == 0 ? ny - w : ny;
  const long long xlim = MODE == 0 ? nx - w : nx;
  const long long x = ox0 + lane;
  // fast path: every cell of the LDS tile is an interior cell
  const bool fast = fy0 >= w && fx0 >= w && fy0 + rows <= ny - w &&
                    fx0 + S <= nx - w;
  const bool periodic = a.periodic_z != 0;

  auto exists = [&](int s) { return periodic || (s >= 0 && s < nz); };
  auto fill = [&](Acc* tile, int s) {
    const int sp = s < 0 ? s + nz : (s >= nz ? s - nz : s);  // |s - sp| <= nz
    stencil3d_fill<T, Acc, MODE>(a, tile, in + (long long)sp * plane,
                                 pl0 + (unsigned)sp, fast, fy0, fx0, lane,
                                 wrow);
  };

  Acc acc[N][kS3Rows];
#pragma unroll
  for (int j = 0; j < N; ++j) {
#pragma unroll
    for (int i = 0; i < kS3Rows; ++i) acc[j][i] = Acc(0);
  }
  const int base = (wrow + w) * S + lane + w;
  [[maybe_unused]] double sum = 0.0;

  // Source planes in march order: s = first, first + DIR, ...; the planes
  // [z0, z1) are among them and exist, the others may not.
  const int first = DIR > 0 ? z0 - RZ : z1 - 1 + RZ;
  const int steps = z1 - z0 + 2 * RZ;
  Acc* cur = buf0;
  Acc* nxt = buf1;
  {
    int s = first;
    while (!exists(s)) s += DIR;
    fill(cur, s);
  }
  __syncthreads();
  for (int i = 0; i < steps; ++i) {
    const int s = first + DIR * i;
    if (exists(s)) {
      if (i + 1 < steps && exists(s + DIR)) fill(nxt, s + DIR);
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const int k = s - DIR * (j - RZ);  // the output plane of dz = j - RZ
        if (k < z0 || k >= z1) continue;   // another chunk's, or none
        for (int t = a.tap_begin[j]; t < a.tap_begin[j + 1]; ++t) {
          const Acc c = stencil_coef<Acc>(a, t);
          const Acc* p = cur + (base + a.tap_off[t]);
#pragma unroll
          for (int r = 0; r < kS3Rows; ++r) {
            acc[j][r] += c * p[r * kS3Waves * S];
          }
        }
      }
      Acc* const t = cur;
      cur = nxt;
      nxt = t;
    }
    // output plane s - DIR * RZ has every term
    const int k = s - DIR * RZ;
    if (k >= z0 && k < z1 && x < xlim) {
      T* o = out + (long long)k * plane;
#pragma unroll
      for (int r = 0; r < kS3Rows; ++r) {
        const long long y = oy0 + wrow + r * kS3Waves;
        if (y < ylim) {
          adj_store<T, Acc>(o + (y * nx + x), acc[N - 1][r]);
          if constexpr (DOT) {
            T stored;
            adj_store<T, Acc>(&stored, acc[N - 1][r]);
            const T* c = in + ((long long)k * plane + y * nx + x);
            sum += (double)adj_load<T, Acc>(c) *
                   (double)adj_load<T, Acc>(&stored);
          }
        }
      }
    }
#pragma unroll
    for (int j = N - 1; j > 0; --j) {
#pragma unroll
      for (int r = 0; r < kS3Rows; ++r) acc[j][r] = acc[j - 1][r];
    }
#pragma unroll
    for (int r = 0; r < kS3Rows; ++r) acc[0][r] = Acc(0);
    // the plane just summed may be refilled, the one just filled read
    __syncthreads();
  }
  if constexpr (DOT) {
    sum = krylov_block_sum(sum);
    if (threadIdx.x == 0) a.partials[blockIdx.x] = sum;
  }
}

template <typename T, typename Acc, int RZ>
void launch_stencil3d_rz(const HaloStencil3dArgs& a, int mode,
                         unsigned blocks, hipStream_t stream) {
  const size_t lds = 2 * (size_t)(kS3TY + 2 * a.w) * (kS3TX + 2 * a.w) *
                     sizeof(Acc);
  dim3 grid(blocks), block(kS3Block);
  if (mode == 0) {
    hipLaunchKernelGGL((halo_stencil3d_kernel<T, Acc, RZ, 0, false>), grid,
                       block, lds, stream, a);
  } else if (mode == 1) {
    hipLaunchKernelGGL((halo_stencil3d_kernel<T, Acc, RZ, 1, false>), grid,
                       block, lds, stream, a);
  } else {
    hipLaunchKernelGGL((halo_stencil3d_kernel<T, Acc, RZ, 0, true>), grid,
                       block, lds, stream, a);
  }
}

template <typename T, typename Acc>
void launch_stencil3d_t(const HaloStencil3dArgs& a, int mode, unsigned blocks,
                        hipStream_t stream) {
  switch (a.rz) {
    case 0: launch_stencil3d_rz<T, Acc, 0>(a, mode, blocks, stream); break;
    case 1: launch_stencil3d_rz<T, Acc, 1>(a, mode, blocks, stream); break;
    case 2: launch_stencil3d_rz<T, Acc, 2>(a, mode, blocks, stream); break;
    default: break;  // rejected by the host-side check in bridge.cpp
  }
}

}  // namespace

hipError_t launch_halo_stencil3d(const HaloStencil3dArgs& a, int mode,
                                 int dt_code, unsigned blocks,
                                 hipStream_t stream) {
  if (blocks == 0) return hipSuccess;
  switch (dt_code) {
    case DT_F32:
      launch_stencil3d_t<float, float>(a, mode, blocks, stream);
      break;
    case DT_F64:
      launch_stencil3d_t<double, double>(a, mode, blocks, stream);
      break;
    case DT_F16:
      launch_stencil3d_t<_Float16, float>(a, mode, blocks, stream);
      break;
    case DT_BF16:
      launch_stencil3d_t<Bf16, float>(a, mode, blocks, stream);
      break;
    default: break;  // rejected by the host-side check in bridge.cpp
  }
  return hipGetLastError();
}
