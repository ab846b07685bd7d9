// Device helpers shared by the three halo stencil kernels (stencil.hip,
// varstencil.hip, stencil3d.hip): how a cell of the LDS tile is fetched on
// the slow path, and the coefficient accessor.  `Args` is the kernel's
// argument struct (HaloStencilArgs, HaloChebArgs, HaloVarStencilArgs or
// HaloStencil3dArgs in kernels.h): the cell helpers use its reg and nx,
// stencil_coef its coef union.
#pragma once

#include "halo_types.h"
#include "kernels.h"

#include <type_traits>

template <typename Acc, typename Args>
__device__ inline Acc stencil_coef(const Args& a, int t) {
  if constexpr (std::is_same<Acc, double>::value) {
    return a.coef.f64[t];
  } else {
    return a.coef.f32[t];
  }
}

// The value the exchange would have put into halo cell (y, x) of plane
// `pl` (= field * levels + level), read from where it comes from.
template <typename T, typename Acc, typename Args>
__device__ inline Acc stencil_halo_cell(const Args& a, const T* plane,
                                        unsigned pl, long long y,
                                        long long x, int k) {
  const StencilRegion& r = a.reg[k];
  if (r.kind == STENCIL_SLOT) {
    const long long s =
        ((long long)pl * r.h + (y - r.ry)) * r.wd + (x - r.rx);
    return adj_load<T, Acc>((const T*)r.buf + s);
  }
  return adj_load<T, Acc>(plane + (y * a.nx + x + r.shift));  // OWN: shift 0
}

// Cell (y, x), y, x >= 0, of the LDS tile of a block that cannot take the
// fast fill; `in` is the input plane and `pl` its index in the slot layout.
// MODE 0 (apply): the cell itself in the interior, the exchanged value in
// the halo, 0 past the plane (such a cell feeds no stored output).
// Otherwise (transposed): the cell itself in the interior, else 0.
// w, ny and nx are the kernel's own copies of a.w, a.ny and a.nx: reading
// them from `a` here changed the transposed kernels' register allocation.
template <typename T, typename Acc, int MODE, typename Args>
__device__ inline Acc stencil_slow_cell(const Args& a, const T* in,
                                        unsigned pl, long long y,
                                        long long x, int w, long long ny,
                                        long long nx) {
  Acc v = Acc(0);
  if (MODE == 0) {
    if (y < ny && x < nx) {
      const int ky = y < w ? 0 : (y >= ny - w ? 2 : 1);
      const int kx = x < w ? 0 : (x >= nx - w ? 2 : 1);
      v = (ky == 1 && kx == 1)
              ? adj_load<T, Acc>(in + (y * nx + x))
              : stencil_halo_cell<T, Acc>(a, in, pl, y, x, ky * 3 + kx);
    }
  } else {
    if (y >= w && y < ny - w && x >= w && x < nx - w) {
      v = adj_load<T, Acc>(in + (y * nx + x));
    }
  }
  return v;
}
