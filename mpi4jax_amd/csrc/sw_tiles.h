// Tile geometry of the single-launch shallow-water step (sw_step1t in
// shallow_water.hip): which tiles are fast, how the fast tiles of a tile
// column are split into the segments a block marches, and which block
// owns what.  Plain C++ (no HIP, no torch) so the kernel, its launcher
// and a host test share one enumeration.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SW_HD __host__ __device__
#else
#define SW_HD
#endif

struct SwFlags {
  // "open" = this halo receives neighbor data (exchange or periodic wrap)
  int south_open, north_open, west_open, east_open;
  // physical walls (reference shallow_water.py:258-262): u column nx-2
  // zeroed on a closed east edge, v row ny-2 zeroed on the north edge
  int east_wall, north_wall;
  // x halos are LOCAL periodic wraps (nproc_x == 1 && periodic), not
  // remote exchanges — lets the fused ring kernel synthesize them
  int x_wrap;
};

// The fast region: cells [jmin, jmax] x [imin, imax) whose whole stencil
// is mask-free (open halos readable, no wall row/column, no hc clamp), so
// the vector kernels run the plain formulas there; each adds its own
// pack-width terms to the test.  Declares the four bounds as locals (a
// macro like SW_BLOCK_MAP, not a struct: every struct or function form
// tried changed the register allocation of the vector kernels).
#define SW_FAST_BOUNDS(ny, nx, f)                                          \
  const int jmin = (f).south_open ? 1 : 2;                                 \
  const int jmax = ((f).north_open && !(f).north_wall) ? ny - 2 : ny - 3;  \
  const int imin = (f).west_open ? 1 : 2;                                  \
  const int imax = ((f).east_open && !(f).east_wall) ? nx - 1 : nx - 2

// XCD-aware block mapping: the dispatcher places block b on XCD b%8, so a
// plain row-major grid scatters adjacent rows across XCDs and every j±1
// stencil read misses that XCD's L2.  This bijective remap of block b of
// T gives each XCD a contiguous band of ids, so neighbor rows are
// L2-resident (MI355X_MICROARCH.md §Workgroup dispatch; speed-only).
// (B = unsigned where the caller has b >= 0 from a branch: shift, no fix-up)
template <typename B>
SW_HD inline int xcd_band_id(B b, int T) {
  const int q8_ = T / 8, r8_ = T % 8, xc_ = b % 8, yc_ = b / 8;
  return (xc_ < r8_ ? xc_ * (q8_ + 1) : r8_ * (q8_ + 1) + (xc_ - r8_) * q8_)
         + yc_;
}

constexpr int kTJ30 = 14;    // output rows per tile
constexpr int kPC30 = 30;    // output pairs (2 cols) per row

// the fast tiles form a rectangle [tr0, tr1] x [tc0, tc1] of the tile
// grid (both predicates are pure bounds); host and device share this.
// Each of its columns is cut into `segs` segments of consecutive tile
// rows, lengths differing by at most one, none longer than the march
// length the caller asked for; one block owns one segment.
struct S1Tiles {
  int bpc, bands, tr0, tr1, tc0, tc1, nfast, nper, nper_pad;
  int segs, nseg;  // segments per fast tile column, and in all
};

SW_HD inline int s1_floordiv(int x, int d) {
  return x >= 0 ? x / d : -((-x + d - 1) / d);
}

SW_HD inline S1Tiles s1_tiles(int ny, int nx, const SwFlags& f, int march) {
  SW_FAST_BOUNDS(ny, nx, f);
  S1Tiles t;
  t.bpc = (nx + 2 * kPC30 - 1) / (2 * kPC30);
  t.bands = (ny + kTJ30 - 1) / kTJ30;
  // rows jb-1 .. jb+TJ all stage19-fast; pairs cb-2 .. cb+2*PC all
  // stage19-fast (i0 + 2 <= imax, i0 + 3 < nx at the last fill pair)
  t.tr0 = s1_floordiv(jmin + 1 + kTJ30 - 1, kTJ30);
  t.tr1 = s1_floordiv(jmax - kTJ30, kTJ30);
  t.tc0 = s1_floordiv(imin + 2 + 2 * kPC30 - 1, 2 * kPC30);
  const int ihi = imax - 2 < nx - 4 ? imax - 2 : nx - 4;
  t.tc1 = s1_floordiv(ihi - 2 * kPC30, 2 * kPC30);
  if (t.tr1 > t.bands - 1) t.tr1 = t.bands - 1;
  if (t.tc1 > t.bpc - 1) t.tc1 = t.bpc - 1;
  const bool any = t.tr0 <= t.tr1 && t.tc0 <= t.tc1;
  t.nfast = any ? (t.tr1 - t.tr0 + 1) * (t.tc1 - t.tc0 + 1) : 0;
  if (!any) {  // canonical empty rectangle: every band is a "top" band
    t.tr0 = t.bands;
    t.tr1 = t.bands - 1;
    t.tc0 = 0;
    t.tc1 = -1;
  }
  t.nper = t.bpc * t.bands - t.nfast;
  // the dispatcher deals blocks to XCDs by raw id mod 8: pad so the fast
  // tiles' XCD bands start on a multiple of 8
  t.nper_pad = (t.nper + 7) / 8 * 8;
  const int rows = t.tr1 - t.tr0 + 1;
  if (march < 1) march = 1;
  t.segs = any ? (rows + march - 1) / march : 0;
  t.nseg = any ? t.segs * (t.tc1 - t.tc0 + 1) : 0;
  return t;
}

// block id -> tile.  Perimeter tiles take the lowest block ids, so their
// longer scalar chains overlap the bulk instead of forming a tail; the
// segments of fast tiles keep the XCD-band remap over their own
// (segment row, tile column) grid.  Returns 0 for a padding block, 1 for
// a perimeter tile, 2 for a segment of fast tiles; *tr is the first tile
// row and *nt the number of tile rows the block owns.
SW_HD inline int s1_block_tile(const S1Tiles& tl, int b, int* tr, int* tc,
                               int* nt) {
  *nt = 1;
  if (b < tl.nper_pad) {
    if (b >= tl.nper) return 0;
    const int top = tl.tr0 * tl.bpc;
    const int bot = (tl.bands - 1 - tl.tr1) * tl.bpc;
    if (b < top) {
      *tr = b / tl.bpc;
      *tc = b % tl.bpc;
    } else if (b < top + bot) {
      *tr = tl.tr1 + 1 + (b - top) / tl.bpc;
      *tc = (b - top) % tl.bpc;
    } else {
      const int w = tl.tc0 + (tl.bpc - 1 - tl.tc1);
      const int u = b - top - bot, c = u % w;
      *tr = tl.tr0 + u / w;
      *tc = c < tl.tc0 ? c : tl.tc1 + 1 + (c - tl.tc0);
    }
    return 1;
  }
  const int bid_ = xcd_band_id((unsigned)(b - tl.nper_pad), tl.nseg);
  const int fw = tl.tc1 - tl.tc0 + 1;
  // even split of the column's rows: the first `rem` segments are one
  // tile longer than the rest
  const int rows = tl.tr1 - tl.tr0 + 1;
  const int len = rows / tl.segs, rem = rows % tl.segs;
  const int s = bid_ / fw;
  *tr = tl.tr0 + s * len + (s < rem ? s : rem);
  *tc = tl.tc0 + bid_ % fw;
  *nt = len + (s < rem ? 1 : 0);
  return 2;
}
