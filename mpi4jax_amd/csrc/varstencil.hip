// Variable-coefficient halo stencil kernel (gfx950) of
// parallel/varstencil.VariableHaloStencil: the contract is next to
// HaloVarStencilArgs in kernels.h.
//
// The coefficients are one (ny, nx) plane per tap, shared by every level,
// so the design point is that their traffic must not grow with the number
// of levels.  A 256-thread workgroup owns one (4 * ROWS) x 64 tile of
// output cells for a chunk of `lpb` consecutive levels of one field.  Wave
// k of the four owns rows k, k + 4, ... of the tile and a lane one column,
// as in stencil.hip, so a thread has ROWS output cells.  It loads the
// ntaps coefficients of each of them ONCE, straight from global memory
// (a wave reads 64 consecutive words of a coefficient row), into
// ROWS * ntaps registers, and keeps them while the block marches over its
// levels.  ROWS is 8 for float accumulation (104 coefficient registers at
// 13 taps) and 4 for double (104 again): no instantiation spills, and all
// run two waves per SIMD (profiles/README.md has the register counts).
//
// Per level the block fills the LDS tile ((4 * ROWS + 2w) rows of 64 + 2w
// values of the accumulate type) exactly as stencil.hip does: tiles whose
// LDS tile lies wholly inside the interior take the register-staged fast
// fill, the others the region-table fill.  The tap loop is fully unrolled
// over the 13 possible taps, so the coefficient registers are indexed
// statically: one LDS word per multiply-add and no coefficient memory.
// Issuing the next level's global loads into the staging registers ahead of
// the current level's tap loop was measured and lost (2 to 11 % slower at
// 16 levels: the registers it holds cost more than the overlap gains), so
// a level's loads are issued right before its LDS stores.
//
// Transposed mode: the LDS tile holds gout (zero outside the interior),
// the tap offsets are negated, and the coefficient of output p and tap t
// is K_t at the source cell p - o_t, loaded from a clamped address and
// replaced by 0 where that cell is not interior; a halo cell of K is never
// read.  Everything after the coefficient load is the same code.
//
// DOT: a thread adds double(centre of the LDS tile) * double(output as
// stored) over its cells, level by level and row by row inside a level,
// from 0; after the march one krylov_block_sum and one store to
// partials[blockIdx.x].

#include "halo_types.h"
#include "kernels.h"
#include "krylov_reduce.h"
#include "stencil_cells.h"

#include <cstdint>

namespace {

constexpr int kVsBlock = kStencilBlock;
constexpr int kVsTX = kStencilTileX;
constexpr int kVsWaves = kVsBlock / kVsTX;
constexpr int kVsT = kVarStencilMaxTaps;

static_assert(kVsBlock == kKrylovBlock,
              "the dot epilogue reduces over a block of the Krylov size");
static_assert(2 * kStencilMaxWidth <= kVsTX,
              "the apron columns are filled by one partial pass");

template <typename T, typename Acc, int ROWS, int MODE, bool DOT>
__global__ __launch_bounds__(kVsBlock) void halo_varstencil_kernel(
    HaloVarStencilArgs a) {
  constexpr int TY = ROWS * kVsWaves;
  constexpr int kFillIts =
      (TY + 2 * kStencilMaxWidth + kVsWaves - 1) / kVsWaves;
  static_assert(!DOT || MODE == 0, "the dot epilogue belongs to apply");
  extern __shared__ __align__(16) unsigned char varstencil_lds[];
  Acc* tile = (Acc*)varstencil_lds;
  const int w = a.w;
  const int S = kVsTX + 2 * w;  // LDS row stride
  const int rows = TY + 2 * w;  // LDS rows
  unsigned b = blockIdx.x;
  const unsigned tix = b % a.tiles_x;
  b /= a.tiles_x;
  const unsigned tiy = b % a.tiles_y;
  b /= a.tiles_y;
  const unsigned ch = b % a.chunks;
  const unsigned f = b / a.chunks;
  const unsigned l0 = ch * a.lpb;
  const unsigned l1 = l0 + a.lpb < a.levels ? l0 + a.lpb : a.levels;
  const long long ny = a.ny, nx = a.nx;
  const long long plane = ny * nx;
  // the output domain: the interior (apply) or the full array (transposed)
  const int org = MODE == 0 ? w : 0;
  const long long oy0 = org + (long long)tiy * TY;
  const long long ox0 = org + (long long)tix * kVsTX;
  const long long fy0 = oy0 - w, fx0 = ox0 - w;  // first cell of the tile
  const int lane = threadIdx.x % kVsTX;
  const int wrow = threadIdx.x / kVsTX;
  const long long ylim = MODE == 0 ? ny - w : ny;
  const long long xlim = MODE == 0 ? nx - w : nx;
  const long long x = ox0 + lane;

  // The thread's coefficients.  Apply: K_t at the output cell, which is
  // interior wherever it is stored; a thread past the edge reads the last
  // interior cell instead and stores nothing.  Transposed: K_t at the
  // source cell, 0 where that is not interior.
  Acc k[kVsT][ROWS];
  {
    const Acc* K = (const Acc*)a.coef;
#pragma unroll
    for (int t = 0; t < kVsT; ++t) {
      if (t >= a.ntaps) continue;  // uniform; keeps k[][] in registers
      const long long sx = MODE == 0 ? x : x - a.tap_dx[t];
      const bool xin = sx >= w && sx < nx - w;
      const long long cx = sx < w ? w : (sx >= nx - w ? nx - w - 1 : sx);
#pragma unroll
      for (int i = 0; i < ROWS; ++i) {
        const long long y = oy0 + wrow + i * kVsWaves;
        const long long sy = MODE == 0 ? y : y - a.tap_dy[t];
        const bool yin = sy >= w && sy < ny - w;
        const long long cy = sy < w ? w : (sy >= ny - w ? ny - w - 1 : sy);
        const Acc v = K[t * plane + cy * nx + cx];
        k[t][i] = (MODE == 0 || (xin && yin)) ? v : Acc(0);
      }
    }
  }

  // fast path: every cell of the LDS tile is an interior cell
  const bool fast = fy0 >= w && fx0 >= w && fy0 + rows <= ny - w &&
                    fx0 + S <= nx - w;
  // staging registers of the fast fill: level l's part of the LDS tile
  T main[kFillIts], side[kFillIts];
  const long long src0 = (fy0 + wrow) * nx + fx0 + lane;
  auto stage = [&](unsigned l) {
    const T* src = (const T*)a.in[f] + ((long long)l * plane + src0);
#pragma unroll
    for (int it = 0; it < kFillIts; ++it) {
      if (wrow + it * kVsWaves < rows) {
        const T* p = src + (long long)it * kVsWaves * nx;
        main[it] = p[0];
        if (lane < 2 * w) side[it] = p[kVsTX];
      }
    }
  };

  const int base = (wrow + w) * S + lane + w;
  [[maybe_unused]] double sum = 0.0;
  for (unsigned l = l0; l < l1; ++l) {
    const T* in = (const T*)a.in[f] + (long long)l * plane;
    T* out = (T*)a.out[f] + (long long)l * plane;
    if (fast) {
      stage(l);
#pragma unroll
      for (int it = 0; it < kFillIts; ++it) {
        const int r = wrow + it * kVsWaves;
        if (r < rows) {
          tile[r * S + lane] = adj_load<T, Acc>(&main[it]);
          if (lane < 2 * w) {
            tile[r * S + kVsTX + lane] = adj_load<T, Acc>(&side[it]);
          }
        }
      }
    } else {
      const unsigned pl = f * a.levels + l;
      for (int r = wrow; r < rows; r += kVsWaves) {
        const long long y = fy0 + r;
        for (int c = lane; c < S; c += kVsTX) {
          tile[r * S + c] =
              stencil_slow_cell<T, Acc, MODE>(a, in, pl, y, fx0 + c, w, ny, nx);
        }
      }
    }
    __syncthreads();

    Acc acc[ROWS];
#pragma unroll
    for (int i = 0; i < ROWS; ++i) acc[i] = Acc(0);
#pragma unroll
    for (int t = 0; t < kVsT; ++t) {
      if (t >= a.ntaps) continue;  // uniform; keeps k[][] in registers
      const int off = a.tap_dy[t] * S + a.tap_dx[t];
      const Acc* p = tile + (base + (MODE == 0 ? off : -off));
#pragma unroll
      for (int i = 0; i < ROWS; ++i) acc[i] += k[t][i] * p[i * kVsWaves * S];
    }

    if (x < xlim) {
#pragma unroll
      for (int i = 0; i < ROWS; ++i) {
        const long long y = oy0 + wrow + i * kVsWaves;
        if (y < ylim) {
          adj_store<T, Acc>(out + (y * nx + x), acc[i]);
          if constexpr (DOT) {
            T stored;
            adj_store<T, Acc>(&stored, acc[i]);
            sum += (double)tile[base + i * kVsWaves * S] *
                   (double)adj_load<T, Acc>(&stored);
          }
        }
      }
    }
    __syncthreads();  // the tile is refilled for the next level
  }
  if constexpr (DOT) {
    sum = krylov_block_sum(sum);
    if (threadIdx.x == 0) a.partials[blockIdx.x] = sum;
  }
}

template <typename T, typename Acc, int ROWS>
void launch_varstencil_t(const HaloVarStencilArgs& a, int mode,
                         unsigned blocks, hipStream_t stream) {
  const size_t lds = (size_t)(ROWS * kVsWaves + 2 * a.w) *
                     (kVsTX + 2 * a.w) * sizeof(Acc);
  dim3 grid(blocks), block(kVsBlock);
  if (mode == 0) {
    hipLaunchKernelGGL((halo_varstencil_kernel<T, Acc, ROWS, 0, false>), grid,
                       block, lds, stream, a);
  } else if (mode == 1) {
    hipLaunchKernelGGL((halo_varstencil_kernel<T, Acc, ROWS, 1, false>), grid,
                       block, lds, stream, a);
  } else {
    hipLaunchKernelGGL((halo_varstencil_kernel<T, Acc, ROWS, 0, true>), grid,
                       block, lds, stream, a);
  }
}

}  // namespace

hipError_t launch_halo_varstencil(const HaloVarStencilArgs& a, int mode,
                                  int dt_code, unsigned blocks,
                                  hipStream_t stream) {
  if (blocks == 0) return hipSuccess;
  switch (dt_code) {
    case DT_F32:
      launch_varstencil_t<float, float, kVarStencilRowsF32>(a, mode, blocks,
                                                            stream);
      break;
    case DT_F64:
      launch_varstencil_t<double, double, kVarStencilRowsF64>(a, mode, blocks,
                                                              stream);
      break;
    case DT_F16:
      launch_varstencil_t<_Float16, float, kVarStencilRowsF32>(a, mode,
                                                               blocks, stream);
      break;
    case DT_BF16:
      launch_varstencil_t<Bf16, float, kVarStencilRowsF32>(a, mode, blocks,
                                                           stream);
      break;
    default: break;  // rejected by the host-side check in bridge.cpp
  }
  return hipGetLastError();
}
