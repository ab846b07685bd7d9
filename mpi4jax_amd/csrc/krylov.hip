// Krylov kernels over HaloStencil fields (gfx950): interior inner
// products and the two vector updates of conjugate gradients.  The
// contract is next to KrylovArgs in kernels.h.
//
// Tiling.  The interior of a plane starts `w` cells into every row, so a
// row of it is not aligned to a wide vector load whatever the dtype; the
// kernels therefore read scalars, 64 consecutive cells of one row per wave
// instruction, which coalesces into whole cache lines but for the row's two
// ends.  A 256-thread block owns the same 32 x 64 tile of interior cells as
// a block of the stencil kernel's mode 0: lane = column, wave k takes rows
// k, k + 4, ..., 8 rows per thread, all loads of a thread issued before
// its first store.
//
// Order of additions of an inner product.  A thread adds the products of
// its rows in row order (k, k + 4, ...), from 0, in float64; cells past
// the interior add nothing.  Then krylov_block_sum (krylov_reduce.h): the
// 64-lane shuffle tree, the four waves in wave order.  Block b stores its
// sum in partials[b].  krylov_finish_kernel, one block: thread t adds
// partials[t], partials[t + 256], ... in that order from 0, then the same
// block sum.  No atomics: the result depends on shape, width and dtype
// only.  For float16, bfloat16 and float32 fields every product is exact
// in float64.

#include "halo_types.h"
#include "kernels.h"
#include "krylov_reduce.h"

#include <cstdint>
#include <type_traits>

namespace {

constexpr int kKrTX = kStencilTileX;
constexpr int kKrTY = kStencilTileY;
constexpr int kKrWaves = kKrylovBlock / kKrTX;
constexpr int kKrRows = kKrTY / kKrWaves;

static_assert(kKrylovBlock == kStencilBlock && kKrTX == 64,
              "one wave per tile row, the stencil's tile grid");

template <typename T>
struct KrAcc {
  using type = float;
};
template <>
struct KrAcc<double> {
  using type = double;
};

// alpha or beta: the quotient in float64, 0 for a zero denominator (an
// iteration past exact convergence changes nothing), rounded once
template <typename Acc>
__device__ inline Acc krylov_ratio(const KrylovArgs& a) {
  const double den = *a.den;
  return (Acc)(den == 0.0 ? 0.0 : *a.num / den);
}

template <typename T, int OP>
__global__ __launch_bounds__(kKrylovBlock) void krylov_kernel(KrylovArgs a) {
  using Acc = typename KrAcc<T>::type;
  unsigned b = blockIdx.x;
  const unsigned tix = b % a.tiles_x;
  b /= a.tiles_x;
  const unsigned tiy = b % a.tiles_y;
  const unsigned pl = b / a.tiles_y;  // field * levels + level
  const unsigned f = pl / a.levels;
  const unsigned l = pl - f * a.levels;
  const long long ny = a.ny, nx = a.nx;
  const int w = a.w;
  const int lane = threadIdx.x % kKrTX;
  const int wrow = threadIdx.x / kKrTX;
  const long long x = w + (long long)tix * kKrTX + lane;
  const long long y0 = w + (long long)tiy * kKrTY + wrow;
  const long long plane = (long long)l * ny * nx;
  const bool col = x < nx - w;
  // rows of this thread inside the interior: y0 + i * kKrWaves < ny - w
  int n = 0;
  if (col && y0 < ny - w) {
    const long long left = (ny - w - y0 + kKrWaves - 1) / kKrWaves;
    n = left < kKrRows ? (int)left : kKrRows;
  }
  const long long first = plane + y0 * nx + x;
  const long long step = (long long)kKrWaves * nx;

  double sum = 0.0;
  if constexpr (OP == KRYLOV_DOT) {
    const T* pa = (const T*)a.a[f] + first;
    const T* pb = (const T*)a.b[f] + first;
    T va[kKrRows], vb[kKrRows];
#pragma unroll
    for (int i = 0; i < kKrRows; ++i) {
      if (i < n) {
        va[i] = pa[i * step];
        vb[i] = pb[i * step];
      }
    }
#pragma unroll
    for (int i = 0; i < kKrRows; ++i) {
      if (i < n) {
        sum += (double)adj_load<T, Acc>(&va[i]) *
               (double)adj_load<T, Acc>(&vb[i]);
      }
    }
  } else if constexpr (OP == KRYLOV_UPDATE) {
    const Acc alpha = krylov_ratio<Acc>(a);
    const Acc* pp = (const Acc*)a.a[f] + first;
    const Acc* pq = (const Acc*)a.b[f] + first;
    Acc* px = (Acc*)a.x[f] + first;
    Acc* pr = (Acc*)a.r[f] + first;
    Acc vp[kKrRows], vq[kKrRows], vx[kKrRows], vr[kKrRows];
#pragma unroll
    for (int i = 0; i < kKrRows; ++i) {
      if (i < n) {
        vp[i] = pp[i * step];
        vq[i] = pq[i * step];
        vx[i] = px[i * step];
        vr[i] = pr[i * step];
      }
    }
#pragma unroll
    for (int i = 0; i < kKrRows; ++i) {
      if (i < n) {
        px[i * step] = vx[i] + alpha * vp[i];
        const Acc rn = vr[i] - alpha * vq[i];
        pr[i * step] = rn;
        sum += (double)rn * (double)rn;
      }
    }
  } else {  // KRYLOV_DIRECTION: p = r + beta p, nothing to reduce
    const Acc beta = krylov_ratio<Acc>(a);
    const Acc* pr = (const Acc*)a.a[f] + first;
    Acc* pp = (Acc*)a.r[f] + first;
    Acc vr[kKrRows], vp[kKrRows];
#pragma unroll
    for (int i = 0; i < kKrRows; ++i) {
      if (i < n) {
        vr[i] = pr[i * step];
        vp[i] = pp[i * step];
      }
    }
#pragma unroll
    for (int i = 0; i < kKrRows; ++i) {
      if (i < n) pp[i * step] = vr[i] + beta * vp[i];
    }
    return;
  }
  sum = krylov_block_sum(sum);
  if (threadIdx.x == 0) a.partials[blockIdx.x] = sum;
}

__global__ __launch_bounds__(kKrylovBlock) void krylov_finish_kernel(
    const double* partials, unsigned n, double* result, double* save) {
  double sum = 0.0;
  for (unsigned i = threadIdx.x; i < n; i += kKrylovBlock) sum += partials[i];
  sum = krylov_block_sum(sum);
  if (threadIdx.x == 0) {
    if (save) *save = *result;
    *result = sum;
  }
}

// The update and direction kernels exist for float and double only.
template <typename T>
void launch_krylov_t(const KrylovArgs& a, int op, unsigned blocks,
                     hipStream_t stream) {
  constexpr bool cg =
      std::is_same<T, float>::value || std::is_same<T, double>::value;
  dim3 grid(blocks), block(kKrylovBlock);
  if (op == KRYLOV_DOT) {
    hipLaunchKernelGGL((krylov_kernel<T, KRYLOV_DOT>), grid, block, 0, stream,
                       a);
  }
  if constexpr (cg) {
    if (op == KRYLOV_UPDATE) {
      hipLaunchKernelGGL((krylov_kernel<T, KRYLOV_UPDATE>), grid, block, 0,
                         stream, a);
    } else if (op == KRYLOV_DIRECTION) {
      hipLaunchKernelGGL((krylov_kernel<T, KRYLOV_DIRECTION>), grid, block,
                         0, stream, a);
    }
  }
}

}  // namespace

hipError_t launch_krylov(const KrylovArgs& a, int op, int dt_code,
                         unsigned blocks, hipStream_t stream) {
  if (blocks == 0) return hipSuccess;
  switch (dt_code) {
    case DT_F32: launch_krylov_t<float>(a, op, blocks, stream); break;
    case DT_F64: launch_krylov_t<double>(a, op, blocks, stream); break;
    case DT_F16: launch_krylov_t<_Float16>(a, op, blocks, stream); break;
    case DT_BF16: launch_krylov_t<Bf16>(a, op, blocks, stream); break;
    default: break;  // rejected by the host-side check in bridge.cpp
  }
  return hipGetLastError();
}

hipError_t launch_krylov_finish(const double* partials, unsigned n,
                                double* result, double* save,
                                hipStream_t stream) {
  hipLaunchKernelGGL(krylov_finish_kernel, dim3(1), dim3(kKrylovBlock), 0,
                     stream, partials, n, result, save);
  return hipGetLastError();
}
