// Host program for tests/test_gpu_sw_marching.py: prints the block -> tile
// enumeration of the single-launch shallow-water step, as the kernel and
// its launcher compute it (csrc/sw_tiles.h).
//
//   sw_tiles_enum NY NX PERIODIC_X MARCH
//
// NY, NX: the local array's shape, halo ring included.  First line:
// "grid <blocks> tr0 tr1 tc0 tc1 nper nper_pad nseg"; then one line per
// block: "<block> <flavour> <first tile row> <tile column> <tile rows>".
#include <cstdio>
#include <cstdlib>

#include "sw_tiles.h"

int main(int argc, char** argv) {
  if (argc != 5) return 2;
  const int ny = std::atoi(argv[1]), nx = std::atoi(argv[2]);
  const int periodic = std::atoi(argv[3]), march = std::atoi(argv[4]);
  // the world-1 model's flags: y closed with a north wall; x either a
  // local periodic wrap or closed with an east wall
  const SwFlags f = {0, 0, periodic, periodic, !periodic, 1, periodic};
  const S1Tiles tl = s1_tiles(ny, nx, f, march);
  const int grid = tl.nper_pad + tl.nseg;
  std::printf("grid %d %d %d %d %d %d %d %d\n", grid, tl.tr0, tl.tr1, tl.tc0,
              tl.tc1, tl.nper, tl.nper_pad, tl.nseg);
  for (int b = 0; b < grid; ++b) {
    int tr = -1, tc = -1, nt = 0;
    const int flavour = s1_block_tile(tl, b, &tr, &tc, &nt);
    std::printf("%d %d %d %d %d\n", b, flavour, tr, tc, nt);
  }
  return 0;
}
