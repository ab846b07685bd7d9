// Halo staging kernels (gfx950): the N-d kernels of
// parallel/halo.HaloExchanger first, then the shallow-water model's 2-D
// ones.
//
// One launch covers every strip of an exchange: up to 8 segments (two
// column strips, two row strips, four corner blocks), each carrying all
// fields and all levels.  A work item is ONE element of the staging
// buffer, so lanes sweep the staging side contiguously; the field side is
// contiguous for row strips (wd = nx - 2w elements per row) and strided
// by nature for column strips (w elements per row).  The same kernel
// body packs (field -> staging) and unpacks (staging -> field); the two
// directions are separate launches so nothing races: a pack launch only
// reads fields, an unpack launch only reads staging, and the unpack's
// segments write disjoint halo cells (a column strip skips the corner
// blocks a corner segment of the same launch owns).
//
// Elements are moved as raw 1/2/4/8-byte words — any dtype of that size
// travels.  Staging indices are 32-bit (the host checks the staging size);
// every offset into a field is 64-bit.
//
// The exchange's adjoint (HaloExchanger.adjoint_) packs the RECEIVE
// windows of the gradient with the same kernel (a third mode stores zeros
// for the rows an unpack skips) and then runs halo_adjoint_acc_kernel, the
// one typed kernel here: send windows overlap, so a field cell collects
// up to 9 terms and the work item is the field cell, which gathers them —
// no atomics, no race, a fixed order of adds.

#include "halo_types.h"
#include "kernels.h"

#include <cstdint>

namespace {

constexpr int kHaloBlock = 256;

// ZPACK (with UNPACK false) is the adjoint's pack: the rows an unpack
// would skip carry a zero word instead of the field's value.
template <typename T, bool UNPACK, bool ZPACK = false>
__global__ __launch_bounds__(kHaloBlock) void halo_nd_kernel(HaloNdArgs a) {
  const unsigned t = blockIdx.x * (unsigned)kHaloBlock + threadIdx.x;
  if (t >= a.total) return;
  // unused segments carry end == total, so they never count
  int k = 0;
#pragma unroll
  for (int i = 0; i < kHaloDirs - 1; ++i) k += t >= a.seg[i].end;
  const HaloNdSeg& sg = a.seg[k];
  const unsigned s = t - sg.start;
  const unsigned c = s % sg.wd;
  const unsigned q = s / sg.wd;
  const unsigned r = q % sg.h;
  const unsigned fl = q / sg.h;
  const unsigned f = fl / a.levels;
  const unsigned l = fl % a.levels;
  if (UNPACK) {
    // corner blocks of a column strip owned by a corner segment
    if (sg.skip_lo && r < (unsigned)a.w) return;
    if (sg.skip_hi && r >= sg.h - (unsigned)a.w) return;
  }
  if (ZPACK) {
    if ((sg.skip_lo && r < (unsigned)a.w) ||
        (sg.skip_hi && r >= sg.h - (unsigned)a.w)) {
      ((T*)sg.buf)[s] = 0;
      return;
    }
  }
  const long long off =
      ((long long)l * a.ny + sg.y0 + r) * a.nx + sg.x0 + c;
  T* field = (T*)a.f[f];
  T* buf = (T*)sg.buf;
  if (UNPACK) {
    field[off] = buf[s];
  } else {
    buf[s] = field[off];
  }
}

template <typename T>
void launch_t(const HaloNdArgs& a, int unpack, hipStream_t stream) {
  dim3 grid((a.total + kHaloBlock - 1) / kHaloBlock), block(kHaloBlock);
  if (unpack == 2) {
    hipLaunchKernelGGL((halo_nd_kernel<T, false, true>), grid, block, 0,
                       stream, a);
  } else if (unpack) {
    hipLaunchKernelGGL((halo_nd_kernel<T, true>), grid, block, 0, stream, a);
  } else {
    hipLaunchKernelGGL((halo_nd_kernel<T, false>), grid, block, 0, stream,
                       a);
  }
}

// ---- adjoint accumulate: typed (halo_types.h), one work item per frame
// cell

template <typename T, typename Acc>
__global__ __launch_bounds__(kHaloBlock) void halo_adjoint_acc_kernel(
    HaloAdjArgs a) {
  const unsigned t = blockIdx.x * (unsigned)kHaloBlock + threadIdx.x;
  if (t >= a.total) return;
  const unsigned fl = t / a.per_level;  // field * levels + level
  unsigned c = t - fl * a.per_level;
  const unsigned f = fl / a.levels;
  const unsigned l = fl - f * a.levels;
  const unsigned nx = (unsigned)a.nx, ny = (unsigned)a.ny;
  const unsigned w2 = 2u * (unsigned)a.w;
  // frame cell -> (y, x); lanes sweep rows of the top / bottom bands
  unsigned y, x;
  if (a.full) {
    y = c / nx;
    x = c - y * nx;
  } else if (c < 2u * a.band) {
    y = c / nx;
    x = c - y * nx;
    if (y >= w2) y += ny - 2u * w2;  // bottom band
  } else {
    c -= 2u * a.band;
    const unsigned sw = 2u * w2;  // west 2w columns, then east 2w
    const unsigned r = c / sw;
    const unsigned xx = c - r * sw;
    y = w2 + r;
    x = xx < w2 ? xx : nx - sw + xx;
  }
  bool zero = false, any = false;
#pragma unroll
  for (int i = 0; i < kHaloDirs; ++i) {
    const HaloAdjSeg& sg = a.seg[i];
    zero |= sg.zero && y - (unsigned)sg.ry < sg.h &&
            x - (unsigned)sg.rx < sg.wd;
  }
  T* p = (T*)a.f[f] + (((long long)l * a.ny + y) * a.nx + x);
  Acc sum = zero ? Acc(0) : adj_load<T, Acc>(p);
  // fixed term order, the entries backwards (corners, S, N, E, W): every
  // executor adds alike, and it is the order in which reverse-mode
  // autodiff through the forward pass's sequence of writes adds them
#pragma unroll
  for (int i = kHaloDirs - 1; i >= 0; --i) {
    const HaloAdjSeg& sg = a.seg[i];
    const unsigned dy = y - (unsigned)sg.sy, dx = x - (unsigned)sg.sx;
    if (sg.acc && dy < sg.h && dx < sg.wd) {
      const unsigned s = (fl * sg.h + dy) * sg.wd + dx;  // < slot size
      sum += adj_load<T, Acc>((const T*)sg.buf + s);
      any = true;
    }
  }
  if (zero || any) adj_store<T, Acc>(p, sum);
}

template <typename T, typename Acc>
void launch_adj_t(const HaloAdjArgs& a, hipStream_t stream) {
  dim3 grid((a.total + kHaloBlock - 1) / kHaloBlock), block(kHaloBlock);
  hipLaunchKernelGGL((halo_adjoint_acc_kernel<T, Acc>), grid, block, 0,
                     stream, a);
}

}  // namespace

void launch_halo_adjoint_acc(const HaloAdjArgs& a, int dt_code,
                             hipStream_t stream) {
  if (a.total == 0) return;
  switch (dt_code) {
    case DT_F32: launch_adj_t<float, float>(a, stream); break;
    case DT_F64: launch_adj_t<double, double>(a, stream); break;
    case DT_F16: launch_adj_t<_Float16, float>(a, stream); break;
    case DT_BF16: launch_adj_t<Bf16, float>(a, stream); break;
    default: break;  // rejected by the host-side check in bridge.cpp
  }
}

void launch_halo_nd(const HaloNdArgs& a, int unpack, int elem_size,
                    hipStream_t stream) {
  if (a.total == 0) return;
  switch (elem_size) {
    case 1: launch_t<uint8_t>(a, unpack, stream); break;
    case 2: launch_t<uint16_t>(a, unpack, stream); break;
    case 4: launch_t<uint32_t>(a, unpack, stream); break;
    case 8: launch_t<uint64_t>(a, unpack, stream); break;
    default: break;  // rejected by the host-side check in bridge.cpp
  }
}

// ------------------------------------------ shallow-water model 2-D halo ops
// The model's own exchange (models/shallow_water.py, sw_exchange): up to 3
// fields of one (ny, nx) level, halo width 1.  One kernel per exchange
// phase instead of torch narrow copies (measured ~110 us/step of
// copyBuffer/elementwise time in the eager halo path).

namespace {

template <typename T>
struct HaloArgs {
  T* f0;
  T* f1;
  T* f2;
  int nf, ny, nx;
  int col;  // for pack/unpack
};

template <typename T>
__device__ inline T* halo_field(const HaloArgs<T>& a, int f) {
  return f == 0 ? a.f0 : (f == 1 ? a.f1 : a.f2);
}

// periodic self-wrap, side 0: east halo col nx-1 <- col 1 ("send west");
// side 1: west halo col 0 <- col nx-2 ("send east")
template <typename T>
__global__ void halo_wrap_kernel(HaloArgs<T> a, int side) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.nf * a.ny) return;
  int f = t / a.ny, j = t % a.ny;
  T* p = halo_field(a, f) + (long long)j * a.nx;
  if (side != 1) p[a.nx - 1] = p[1];
  if (side != 0) p[0] = p[a.nx - 2];  // side 2 = both wraps in one launch
}

template <typename T>
__global__ void pack_cols_kernel(HaloArgs<T> a, T* buf) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.nf * a.ny) return;
  int f = t / a.ny, j = t % a.ny;
  buf[t] = halo_field(a, f)[(long long)j * a.nx + a.col];
}

template <typename T>
__global__ void unpack_cols_kernel(HaloArgs<T> a, const T* buf) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.nf * a.ny) return;
  int f = t / a.ny, j = t % a.ny;
  halo_field(a, f)[(long long)j * a.nx + a.col] = buf[t];
}

template <typename T>
HaloArgs<T> make_halo_args(void* const* fields, int nf, long long ny,
                           long long nx, long long col) {
  HaloArgs<T> a;
  a.f0 = (T*)fields[0];
  a.f1 = nf > 1 ? (T*)fields[1] : (T*)fields[0];
  a.f2 = nf > 2 ? (T*)fields[2] : (T*)fields[0];
  a.nf = nf;
  a.ny = (int)ny;
  a.nx = (int)nx;
  a.col = (int)col;
  return a;
}

int halo_grid(int n) { return (n + kHaloBlock - 1) / kHaloBlock; }

}  // namespace

void launch_halo_wrap(void* const* fields, int nf, long long ny,
                      long long nx, int side, int is_double,
                      hipStream_t stream) {
  int n = nf * (int)ny;
  if (is_double) {
    auto a = make_halo_args<double>(fields, nf, ny, nx, 0);
    hipLaunchKernelGGL(halo_wrap_kernel<double>, dim3(halo_grid(n)),
                       dim3(kHaloBlock), 0, stream, a, side);
  } else {
    auto a = make_halo_args<float>(fields, nf, ny, nx, 0);
    hipLaunchKernelGGL(halo_wrap_kernel<float>, dim3(halo_grid(n)),
                       dim3(kHaloBlock), 0, stream, a, side);
  }
}

void launch_pack_cols(void* buf, void* const* fields, int nf, long long ny,
                      long long nx, long long col, int is_double,
                      hipStream_t stream) {
  int n = nf * (int)ny;
  if (is_double) {
    auto a = make_halo_args<double>(fields, nf, ny, nx, col);
    hipLaunchKernelGGL(pack_cols_kernel<double>, dim3(halo_grid(n)),
                       dim3(kHaloBlock), 0, stream, a, (double*)buf);
  } else {
    auto a = make_halo_args<float>(fields, nf, ny, nx, col);
    hipLaunchKernelGGL(pack_cols_kernel<float>, dim3(halo_grid(n)),
                       dim3(kHaloBlock), 0, stream, a, (float*)buf);
  }
}

void launch_unpack_cols(void* const* fields, const void* buf, int nf,
                        long long ny, long long nx, long long col,
                        int is_double, hipStream_t stream) {
  int n = nf * (int)ny;
  if (is_double) {
    auto a = make_halo_args<double>(fields, nf, ny, nx, col);
    hipLaunchKernelGGL(unpack_cols_kernel<double>, dim3(halo_grid(n)),
                       dim3(kHaloBlock), 0, stream, a, (const double*)buf);
  } else {
    auto a = make_halo_args<float>(fields, nf, ny, nx, col);
    hipLaunchKernelGGL(unpack_cols_kernel<float>, dim3(halo_grid(n)),
                       dim3(kHaloBlock), 0, stream, a, (const float*)buf);
  }
}

// corner pack/unpack for the single-group halo exchange: buf layout is
// [diag d][field f] with d: 0=to-SW/from-NE, 1=to-SE/from-NW,
// 2=to-NW/from-SE, 3=to-NE/from-SW (matching parallel/grid.py halo_plan).
namespace {

template <typename T>
__global__ void pack_corners_kernel(HaloArgs<T> a, T* buf) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 4 * a.nf) return;
  int d = t / a.nf, f = t % a.nf;
  const int ny = a.ny, nx = a.nx;
  int j = (d < 2) ? 1 : ny - 2;
  int i = (d == 0 || d == 2) ? 1 : nx - 2;
  buf[t] = halo_field(a, f)[(long long)j * nx + i];
}

template <typename T>
__global__ void unpack_corners_kernel(HaloArgs<T> a, const T* buf,
                                      int mask) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 4 * a.nf) return;
  int d = t / a.nf, f = t % a.nf;
  if (!(mask & (1 << d))) return;
  const int ny = a.ny, nx = a.nx;
  // recv cells: d0 (ny-1,nx-1), d1 (ny-1,0), d2 (0,nx-1), d3 (0,0)
  int j = (d < 2) ? ny - 1 : 0;
  int i = (d == 0 || d == 2) ? nx - 1 : 0;
  halo_field(a, f)[(long long)j * nx + i] = buf[t];
}

// merged staging: wrap + both column packs + corner pack in ONE launch
// (work layout [wrap | cb0 | cb1 | corners]); see kernels.h for the
// contract.  All segments touch disjoint cells: wrap writes halo cols
// 0/nx-1, col packs read interior cols (1/nx-2), corner pack reads
// interior corner cells.
template <typename T>
struct HaloXArgs {
  T* f0;
  T* f1;
  T* f2;
  int nf, ny, nx;
  T* cb0;
  T* cb1;
  T* cor;
  int c0, c1;
  int wrap_side;  // -1 none, 0 east<-1, 1 west<-nx-2, 2 both
  int cor_mask;
};

template <typename T>
__device__ inline T* hx_field(const HaloXArgs<T>& a, int f) {
  return f == 0 ? a.f0 : (f == 1 ? a.f1 : a.f2);
}

template <typename T>
__global__ void pack_halo_kernel(HaloXArgs<T> a) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int ncol = a.nf * a.ny;
  if (t < ncol) {
    if (a.wrap_side < 0) return;
    int f = t / a.ny, j = t % a.ny;
    T* p = hx_field(a, f) + (long long)j * a.nx;
    if (a.wrap_side != 1) p[a.nx - 1] = p[1];
    if (a.wrap_side != 0) p[0] = p[a.nx - 2];
    return;
  }
  t -= ncol;
  if (t < 2 * ncol) {
    T* buf = t < ncol ? a.cb0 : a.cb1;
    int col = t < ncol ? a.c0 : a.c1;
    if (!buf) return;
    int s = t % ncol;
    int f = s / a.ny, j = s % a.ny;
    buf[s] = hx_field(a, f)[(long long)j * a.nx + col];
    return;
  }
  t -= 2 * ncol;
  if (t >= 4 * a.nf || !a.cor) return;
  int d = t / a.nf, f = t % a.nf;
  int j = (d < 2) ? 1 : a.ny - 2;
  int i = (d == 0 || d == 2) ? 1 : a.nx - 2;
  a.cor[t] = hx_field(a, f)[(long long)j * a.nx + i];
}

// which corner diagonal writes cell (j in {0, ny-1}, col in {0, nx-1}):
// d0 (ny-1,nx-1), d1 (ny-1,0), d2 (0,nx-1), d3 (0,0)
__device__ inline int corner_diag(bool top_row, bool east_col) {
  return top_row ? (east_col ? 0 : 1) : (east_col ? 2 : 3);
}

template <typename T>
__global__ void unpack_halo_kernel(HaloXArgs<T> a) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int ncol = a.nf * a.ny;
  if (t < 2 * ncol) {
    const T* buf = t < ncol ? a.cb0 : a.cb1;
    int col = t < ncol ? a.c0 : a.c1;
    if (!buf) return;
    int s = t % ncol;
    int f = s / a.ny, j = s % a.ny;
    if ((j == 0 || j == a.ny - 1) && a.cor) {
      // the corner segment of this same launch owns this cell
      int d = corner_diag(j == a.ny - 1, col == a.nx - 1);
      if (a.cor_mask & (1 << d)) return;
    }
    hx_field(a, f)[(long long)j * a.nx + col] = buf[s];
    return;
  }
  t -= 2 * ncol;
  if (t >= 4 * a.nf || !a.cor) return;
  int d = t / a.nf, f = t % a.nf;
  if (!(a.cor_mask & (1 << d))) return;
  int j = (d < 2) ? a.ny - 1 : 0;
  int i = (d == 0 || d == 2) ? a.nx - 1 : 0;
  hx_field(a, f)[(long long)j * a.nx + i] = a.cor[t];
}

template <typename T>
HaloXArgs<T> make_hx_args(void* const* fields, int nf, long long ny,
                          long long nx, int wrap_side, void* cb0,
                          long long c0, void* cb1, long long c1, void* cor,
                          int cor_mask) {
  HaloXArgs<T> a;
  a.f0 = (T*)fields[0];
  a.f1 = nf > 1 ? (T*)fields[1] : (T*)fields[0];
  a.f2 = nf > 2 ? (T*)fields[2] : (T*)fields[0];
  a.nf = nf;
  a.ny = (int)ny;
  a.nx = (int)nx;
  a.cb0 = (T*)cb0;
  a.cb1 = (T*)cb1;
  a.cor = (T*)cor;
  a.c0 = (int)c0;
  a.c1 = (int)c1;
  a.wrap_side = wrap_side;
  a.cor_mask = cor_mask;
  return a;
}

}  // namespace

void launch_pack_corners(void* buf, void* const* fields, int nf,
                         long long ny, long long nx, int is_double,
                         hipStream_t stream) {
  int n = 4 * nf;
  if (is_double) {
    auto a = make_halo_args<double>(fields, nf, ny, nx, 0);
    hipLaunchKernelGGL(pack_corners_kernel<double>, dim3(1), dim3(64), 0,
                       stream, a, (double*)buf);
  } else {
    auto a = make_halo_args<float>(fields, nf, ny, nx, 0);
    hipLaunchKernelGGL(pack_corners_kernel<float>, dim3(1), dim3(64), 0,
                       stream, a, (float*)buf);
  }
  (void)n;
}

void launch_unpack_corners(void* const* fields, const void* buf, int nf,
                           long long ny, long long nx, int mask,
                           int is_double, hipStream_t stream) {
  if (is_double) {
    auto a = make_halo_args<double>(fields, nf, ny, nx, 0);
    hipLaunchKernelGGL(unpack_corners_kernel<double>, dim3(1), dim3(64), 0,
                       stream, a, (const double*)buf, mask);
  } else {
    auto a = make_halo_args<float>(fields, nf, ny, nx, 0);
    hipLaunchKernelGGL(unpack_corners_kernel<float>, dim3(1), dim3(64), 0,
                       stream, a, (const float*)buf, mask);
  }
}

void launch_pack_halo(void* const* fields, int nf, long long ny,
                      long long nx, int wrap_side, void* cb0, long long c0,
                      void* cb1, long long c1, void* cor, int is_double,
                      hipStream_t stream) {
  int n = 3 * nf * (int)ny + 4 * nf;
  if (is_double) {
    auto a = make_hx_args<double>(fields, nf, ny, nx, wrap_side, cb0, c0,
                                  cb1, c1, cor, 0);
    hipLaunchKernelGGL(pack_halo_kernel<double>, dim3(halo_grid(n)),
                       dim3(kHaloBlock), 0, stream, a);
  } else {
    auto a = make_hx_args<float>(fields, nf, ny, nx, wrap_side, cb0, c0,
                                 cb1, c1, cor, 0);
    hipLaunchKernelGGL(pack_halo_kernel<float>, dim3(halo_grid(n)),
                       dim3(kHaloBlock), 0, stream, a);
  }
}

void launch_unpack_halo(void* const* fields, int nf, long long ny,
                        long long nx, void* cb0, long long c0, void* cb1,
                        long long c1, void* cor, int cor_mask,
                        int is_double, hipStream_t stream) {
  int n = 2 * nf * (int)ny + 4 * nf;
  if (is_double) {
    auto a = make_hx_args<double>(fields, nf, ny, nx, -1, cb0, c0, cb1, c1,
                                  cor, cor_mask);
    hipLaunchKernelGGL(unpack_halo_kernel<double>, dim3(halo_grid(n)),
                       dim3(kHaloBlock), 0, stream, a);
  } else {
    auto a = make_hx_args<float>(fields, nf, ny, nx, -1, cb0, c0, cb1, c1,
                                 cor, cor_mask);
    hipLaunchKernelGGL(unpack_halo_kernel<float>, dim3(halo_grid(n)),
                       dim3(kHaloBlock), 0, stream, a);
  }
}
