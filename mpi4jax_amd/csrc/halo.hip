// N-d halo staging kernels for parallel/halo.HaloExchanger (gfx950).
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

#include "kernels.h"

#include <cstdint>

namespace {

constexpr int kHaloBlock = 256;

template <typename T, bool UNPACK>
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
  if (unpack) {
    hipLaunchKernelGGL((halo_nd_kernel<T, true>), grid, block, 0, stream, a);
  } else {
    hipLaunchKernelGGL((halo_nd_kernel<T, false>), grid, block, 0, stream,
                       a);
  }
}

}  // namespace

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
