// Slot and frame geometry of parallel/halo.HaloExchanger — plain C++, no
// HIP and no torch, shared by halo_exchange_nd and halo_adjoint_nd in
// bridge.cpp.  Every product is formed in 64 bits; the callers check the
// results against the 32-bit index range of the kernels.
#pragma once

#include <cstdint>

constexpr int kHaloGeomDirs = 8;

// Entry i is direction i of halo.DIRECTIONS as (dy, dx): columns W, E,
// rows N, S, then the diagonals (-1,-1), (-1,1), (1,-1), (1,1).
struct HaloGeom {
  int64_t slot_off[kHaloGeomDirs + 1];  // staging offsets, in elements
  int64_t sy[kHaloGeomDirs], sx[kHaloGeomDirs];  // send-window origin
  int64_t ry[kHaloGeomDirs], rx[kHaloGeomDirs];  // receive-window origin
  int64_t hh[kHaloGeomDirs], ww[kHaloGeomDirs];  // window size
  int64_t total;                                 // == slot_off[8]
};

// Needs w >= 1, ny >= 3*w, nx >= 3*w, nf >= 1, levels >= 1.
inline HaloGeom halo_geometry(int64_t nf, int64_t levels, int64_t ny,
                              int64_t nx, int64_t w) {
  static const int64_t dirs[kHaloGeomDirs][2] = {
      {0, -1}, {0, 1}, {1, 0}, {-1, 0}, {-1, -1}, {-1, 1}, {1, -1}, {1, 1}};
  HaloGeom g;
  g.slot_off[0] = 0;
  for (int i = 0; i < kHaloGeomDirs; ++i) {
    const int64_t dy = dirs[i][0], dx = dirs[i][1];
    // y: a column strip (dy == 0) is full height
    g.sy[i] = dy < 0 ? w : (dy > 0 ? ny - 2 * w : 0);
    g.ry[i] = dy < 0 ? ny - w : 0;
    g.hh[i] = dy != 0 ? w : ny;
    // x: a row strip (dx == 0) covers the interior columns
    g.sx[i] = dx < 0 ? w : (dx > 0 ? nx - 2 * w : w);
    g.rx[i] = dx < 0 ? nx - w : (dx > 0 ? 0 : w);
    g.ww[i] = dx != 0 ? w : nx - 2 * w;
    g.slot_off[i + 1] = g.slot_off[i] + nf * levels * g.hh[i] * g.ww[i];
  }
  g.total = g.slot_off[kHaloGeomDirs];
  return g;
}

// The frame of one (ny, nx) level: the cells within 2*w of an edge — every
// cell an exchange reads or writes.  Work layout per level: rows [0, 2w)
// and [ny - 2w, ny) over all nx columns (2 * band items), then rows
// [2w, ny - 2w) over the 2w + 2w side columns.  An axis shorter than 4*w
// makes the bands overlap, so then the frame is the whole level (full).
// HaloExchanger.__init__ (parallel/halo.py, _adj_work) repeats per_level
// to refuse an oversized adjoint before the call: change the two together.
struct HaloFrame {
  int full;
  int64_t band;       // 2*w*nx: items of the top (or bottom) band
  int64_t per_level;  // frame cells of one level
};

inline HaloFrame halo_frame(int64_t ny, int64_t nx, int64_t w) {
  HaloFrame fr;
  fr.full = ny < 4 * w || nx < 4 * w;
  fr.band = 2 * w * nx;
  fr.per_level = fr.full ? ny * nx : 2 * fr.band + (ny - 4 * w) * 4 * w;
  return fr;
}
