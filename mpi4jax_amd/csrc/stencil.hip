// Fused halo stencil kernel (gfx950) of parallel/stencil.HaloStencil: the
// contract is next to HaloStencilArgs in kernels.h.
//
// A 256-thread workgroup owns a 32 x 64 tile of output cells of one
// (ny, nx) plane.  The LDS tile is (32 + 2w) rows of (64 + 2w) values of
// the accumulate type.  Wave k of the four fills rows k, k + 4, ...: its 64
// lanes read 64 consecutive cells of a row, and lanes [0, 2w) read the rest
// of the row in a second pass.  In the tap loop a wave again reads 64
// consecutive LDS words of one row per instruction, whatever the tap's
// offset and whatever the row stride, so no access has a bank conflict and
// the tile needs no padding.  A thread keeps 8 outputs (rows k, k + 4, ...
// of its column) in registers, so a coefficient and a tap offset are
// fetched once per 8 multiply-adds.
//
// The taps, their coefficients and the region table travel in the
// kernel-argument struct.  Every output is the sum, from 0 and in the order
// of the tap list, of coefficient * value: no atomics, one fixed order.
// Tiles whose LDS tile lies wholly inside the plane's interior (all but
// the outermost ring of tiles) take the straight fill and never look at
// the region table.
//
// DOT (apply only, launch_halo_stencil_dot) adds an epilogue after the
// stores: the block's part of in . out over its output cells, in float64.
// A thread adds, in the order of its 8 rows and from 0,
// double(centre of the LDS tile) * double(the output as stored, so after
// the rounding of a float16 / bfloat16 store); a lane or a row past the
// interior adds nothing.  Then krylov_block_sum (krylov_reduce.h: shuffle
// tree, waves in order) and one store to partials[blockIdx.x].  Without
// DOT the kernel is what it was: every added statement is under
// `if constexpr (DOT)`.
//
// CHEB (apply only, float32 / float64, launch_halo_stencil_cheb) turns the
// launch into one Chebyshev iteration (HaloChebArgs in kernels.h): `in` is
// the direction d, the tap loop leaves q = A d in registers, and the store
// becomes x += d, r -= q, out = c1 * d + c2 * r on the thread's interior
// cells, with d at the centre taken from the LDS tile.  The thread's x
// and r loads are issued before the tap loop so that their latency hides
// under it.  Every added statement is under `if constexpr (CHEB)` (the
// two register arrays are declared outside it, one unused element each
// otherwise, and the plain store is its else branch), and only then does
// the kernel take the longer argument struct: the other instantiations
// compile to the instructions they had.

#include "halo_types.h"
#include "kernels.h"
#include "krylov_reduce.h"

#include <cstdint>
#include <type_traits>

namespace {

constexpr int kStBlock = kStencilBlock;
constexpr int kStTX = kStencilTileX;
constexpr int kStTY = kStencilTileY;
constexpr int kStWaves = kStBlock / kStTX;  // rows filled / summed per pass
constexpr int kStRows = kStTY / kStWaves;   // outputs per thread
// LDS rows a wave fills at the largest width
constexpr int kStFillIts =
    (kStTY + 2 * kStencilMaxWidth + kStWaves - 1) / kStWaves;

static_assert(kStBlock % kStTX == 0 && kStTY % kStWaves == 0,
              "tile shape must divide over the block");
static_assert(2 * kStencilMaxWidth <= kStTX,
              "the apron columns are filled by one partial pass");
static_assert(kStBlock == kKrylovBlock,
              "the dot epilogue reduces over a block of the Krylov size");

template <typename Acc>
__device__ inline Acc stencil_coef(const HaloStencilArgs& a, int t);
template <>
__device__ inline float stencil_coef<float>(const HaloStencilArgs& a, int t) {
  return a.coef.f32[t];
}
template <>
__device__ inline double stencil_coef<double>(const HaloStencilArgs& a,
                                              int t) {
  return a.coef.f64[t];
}

// The value the exchange would have put into halo cell (y, x) of plane
// `pl` (= field * levels + level), read from where it comes from.
template <typename T, typename Acc>
__device__ inline Acc stencil_halo_cell(const HaloStencilArgs& a,
                                        const T* plane, unsigned pl,
                                        long long y, long long x, int k) {
  const StencilRegion& r = a.reg[k];
  if (r.kind == STENCIL_SLOT) {
    const long long s =
        ((long long)pl * r.h + (y - r.ry)) * r.wd + (x - r.rx);
    return adj_load<T, Acc>((const T*)r.buf + s);
  }
  return adj_load<T, Acc>(plane + (y * a.nx + x + r.shift));  // OWN: shift 0
}

template <typename T, typename Acc, int MODE, bool DOT = false,
          bool CHEB = false>
__global__ __launch_bounds__(kStBlock) void halo_stencil_kernel(
    std::conditional_t<CHEB, HaloChebArgs, HaloStencilArgs> a) {
  extern __shared__ __align__(16) unsigned char stencil_lds[];
  Acc* tile = (Acc*)stencil_lds;
  const int w = a.w;
  const int S = kStTX + 2 * w;     // LDS row stride
  const int rows = kStTY + 2 * w;  // LDS rows
  unsigned b = blockIdx.x;
  const unsigned tix = b % a.tiles_x;
  b /= a.tiles_x;
  const unsigned tiy = b % a.tiles_y;
  const unsigned pl = b / a.tiles_y;  // field * levels + level
  const unsigned f = pl / a.levels;
  const unsigned l = pl - f * a.levels;
  const long long ny = a.ny, nx = a.nx;
  const T* in = (const T*)a.in[f] + (long long)l * ny * nx;
  T* out = (T*)a.out[f] + (long long)l * ny * nx;
  // the output domain: the interior (apply) or the full array (transposed)
  const int org = MODE == 0 ? w : 0;
  const long long oy0 = org + (long long)tiy * kStTY;
  const long long ox0 = org + (long long)tix * kStTX;
  const long long fy0 = oy0 - w, fx0 = ox0 - w;  // first cell of the tile
  const int lane = threadIdx.x % kStTX;
  const int wrow = threadIdx.x / kStTX;

  // fast path: every cell of the LDS tile is an interior cell
  const bool fast = fy0 >= w && fx0 >= w && fy0 + rows <= ny - w &&
                    fx0 + S <= nx - w;
  if (fast) {
    // all of a wave's global loads are issued before the first LDS store,
    // so their latencies overlap instead of adding up row by row
    T main[kStFillIts], side[kStFillIts];
    const T* src = in + ((fy0 + wrow) * nx + fx0 + lane);
#pragma unroll
    for (int it = 0; it < kStFillIts; ++it) {
      if (wrow + it * kStWaves < rows) {
        const T* p = src + (long long)it * kStWaves * nx;
        main[it] = p[0];
        if (lane < 2 * w) side[it] = p[kStTX];
      }
    }
#pragma unroll
    for (int it = 0; it < kStFillIts; ++it) {
      const int r = wrow + it * kStWaves;
      if (r < rows) {
        tile[r * S + lane] = adj_load<T, Acc>(&main[it]);
        if (lane < 2 * w) {
          tile[r * S + kStTX + lane] = adj_load<T, Acc>(&side[it]);
        }
      }
    }
  } else {
    for (int r = wrow; r < rows; r += kStWaves) {
      const long long y = fy0 + r;
      for (int c = lane; c < S; c += kStTX) {
        const long long x = fx0 + c;
        Acc v = Acc(0);
        if (MODE == 0) {
          // y, x >= 0 here; cells past the plane feed no stored output
          if (y < ny && x < nx) {
            const int ky = y < w ? 0 : (y >= ny - w ? 2 : 1);
            const int kx = x < w ? 0 : (x >= nx - w ? 2 : 1);
            v = (ky == 1 && kx == 1)
                    ? adj_load<T, Acc>(in + (y * nx + x))
                    : stencil_halo_cell<T, Acc>(a, in, pl, y, x,
                                                ky * 3 + kx);
          }
        } else {
          if (y >= w && y < ny - w && x >= w && x < nx - w) {
            v = adj_load<T, Acc>(in + (y * nx + x));
          }
        }
        tile[r * S + c] = v;
      }
    }
  }
  __syncthreads();

  // CHEB: this thread's cells of x and r, loaded ahead of the tap loop
  [[maybe_unused]] T cheb_x[CHEB ? kStRows : 1];
  [[maybe_unused]] T cheb_r[CHEB ? kStRows : 1];
  if constexpr (CHEB) {
    static_assert(MODE == 0 && !DOT && std::is_same<T, Acc>::value,
                  "the Chebyshev epilogue belongs to apply in f32 / f64");
    const long long cx = ox0 + lane;
    if (cx < nx - w) {
      const long long pl0 = (long long)l * ny * nx;
      const T* px = (const T*)a.x[f] + pl0;
      const T* pr = (const T*)a.r[f] + pl0;
#pragma unroll
      for (int i = 0; i < kStRows; ++i) {
        const long long cy = oy0 + wrow + i * kStWaves;
        if (cy < ny - w) {
          cheb_x[i] = px[cy * nx + cx];
          cheb_r[i] = pr[cy * nx + cx];
        }
      }
    }
  }

  Acc acc[kStRows];
#pragma unroll
  for (int i = 0; i < kStRows; ++i) acc[i] = Acc(0);
  const int base = (wrow + w) * S + lane + w;
  for (int t = 0; t < a.ntaps; ++t) {
    const Acc k = stencil_coef<Acc>(a, t);
    const Acc* p = tile + (base + a.tap_off[t]);
#pragma unroll
    for (int i = 0; i < kStRows; ++i) acc[i] += k * p[i * kStWaves * S];
  }

  const long long ylim = MODE == 0 ? ny - w : ny;
  const long long xlim = MODE == 0 ? nx - w : nx;
  const long long x = ox0 + lane;
  if constexpr (CHEB) {
    if (x < xlim) {
      const Acc c1 = (Acc)a.c1, c2 = (Acc)a.c2;
      const long long pl0 = (long long)l * ny * nx;
      T* px = (T*)a.x[f] + pl0;
      T* pr = (T*)a.r[f] + pl0;
#pragma unroll
      for (int i = 0; i < kStRows; ++i) {
        const long long y = oy0 + wrow + i * kStWaves;
        if (y < ylim) {
          const Acc d = tile[base + i * kStWaves * S];
          const Acc rn = cheb_r[i] - acc[i];
          px[y * nx + x] = cheb_x[i] + d;
          pr[y * nx + x] = rn;
          out[y * nx + x] = c1 * d + c2 * rn;
        }
      }
    }
  } else if (x < xlim) {
#pragma unroll
    for (int i = 0; i < kStRows; ++i) {
      const long long y = oy0 + wrow + i * kStWaves;
      if (y < ylim) adj_store<T, Acc>(out + (y * nx + x), acc[i]);
    }
  }
  if constexpr (DOT) {
    static_assert(MODE == 0, "the dot epilogue belongs to apply");
    double sum = 0.0;
    if (x < xlim) {
#pragma unroll
      for (int i = 0; i < kStRows; ++i) {
        if (oy0 + wrow + i * kStWaves < ylim) {
          T stored;
          adj_store<T, Acc>(&stored, acc[i]);
          sum += (double)tile[base + i * kStWaves * S] *
                 (double)adj_load<T, Acc>(&stored);
        }
      }
    }
    sum = krylov_block_sum(sum);
    if (threadIdx.x == 0) a.partials[blockIdx.x] = sum;
  }
}

template <typename T, typename Acc>
void launch_stencil_t(const HaloStencilArgs& a, int mode, unsigned blocks,
                      hipStream_t stream) {
  const size_t lds = (size_t)(kStTY + 2 * a.w) * (kStTX + 2 * a.w) *
                     sizeof(Acc);
  dim3 grid(blocks), block(kStBlock);
  if (mode == 0) {
    hipLaunchKernelGGL((halo_stencil_kernel<T, Acc, 0>), grid, block, lds,
                       stream, a);
  } else {
    hipLaunchKernelGGL((halo_stencil_kernel<T, Acc, 1>), grid, block, lds,
                       stream, a);
  }
}

template <typename T, typename Acc>
void launch_stencil_dot_t(const HaloStencilArgs& a, unsigned blocks,
                          hipStream_t stream) {
  const size_t lds = (size_t)(kStTY + 2 * a.w) * (kStTX + 2 * a.w) *
                     sizeof(Acc);
  hipLaunchKernelGGL((halo_stencil_kernel<T, Acc, 0, true>), dim3(blocks),
                     dim3(kStBlock), lds, stream, a);
}

template <typename T>
void launch_stencil_cheb_t(const HaloChebArgs& a, unsigned blocks,
                           hipStream_t stream) {
  const size_t lds = (size_t)(kStTY + 2 * a.w) * (kStTX + 2 * a.w) *
                     sizeof(T);
  hipLaunchKernelGGL((halo_stencil_kernel<T, T, 0, false, true>),
                     dim3(blocks), dim3(kStBlock), lds, stream, a);
}

}  // namespace

hipError_t launch_halo_stencil_cheb(const HaloChebArgs& a, int dt_code,
                                    unsigned blocks, hipStream_t stream) {
  if (blocks == 0) return hipSuccess;
  switch (dt_code) {
    case DT_F32: launch_stencil_cheb_t<float>(a, blocks, stream); break;
    case DT_F64: launch_stencil_cheb_t<double>(a, blocks, stream); break;
    default: break;  // rejected by the host-side check in bridge.cpp
  }
  return hipGetLastError();
}

hipError_t launch_halo_stencil_dot(const HaloStencilArgs& a, int dt_code,
                                   unsigned blocks, hipStream_t stream) {
  if (blocks == 0) return hipSuccess;
  switch (dt_code) {
    case DT_F32: launch_stencil_dot_t<float, float>(a, blocks, stream); break;
    case DT_F64:
      launch_stencil_dot_t<double, double>(a, blocks, stream);
      break;
    case DT_F16:
      launch_stencil_dot_t<_Float16, float>(a, blocks, stream);
      break;
    case DT_BF16: launch_stencil_dot_t<Bf16, float>(a, blocks, stream); break;
    default: break;  // rejected by the host-side check in bridge.cpp
  }
  return hipGetLastError();
}

hipError_t launch_halo_stencil(const HaloStencilArgs& a, int mode,
                               int dt_code, unsigned blocks,
                               hipStream_t stream) {
  if (blocks == 0) return hipSuccess;
  switch (dt_code) {
    case DT_F32: launch_stencil_t<float, float>(a, mode, blocks, stream); break;
    case DT_F64:
      launch_stencil_t<double, double>(a, mode, blocks, stream);
      break;
    case DT_F16:
      launch_stencil_t<_Float16, float>(a, mode, blocks, stream);
      break;
    case DT_BF16: launch_stencil_t<Bf16, float>(a, mode, blocks, stream); break;
    default: break;  // rejected by the host-side check in bridge.cpp
  }
  return hipGetLastError();
}
