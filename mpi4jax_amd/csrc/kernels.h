// CDNA4 device kernels (gfx950) — C ABI, torch-free.
#pragma once

#include <hip/hip_runtime.h>

// dtype codes shared between bridge.cpp and kernels.hip
enum DtCode : int {
  DT_F32 = 0,
  DT_F64 = 1,
  DT_F16 = 2,
  DT_BF16 = 3,
  DT_I8 = 4,
  DT_U8 = 5,
  DT_I32 = 6,
  DT_I64 = 7,
};

enum OpCode : int {  // matches ncclRedOp_t for the first four
  OPC_SUM = 0,
  OPC_PROD = 1,
  OPC_MAX = 2,
  OPC_MIN = 3,
  // kernel-only codes (never passed to an RCCL collective — RCCL has no
  // bitwise reductions; these ride the p2p+combine compositions)
  OPC_BAND = 5,
  OPC_BOR = 6,
  OPC_BXOR = 7,
};

// dst[i] = a[i] (op) b[i], grid-strided, enqueued on `stream`
void launch_combine(void* dst, const void* a, const void* b, long long n,
                    int dt_code, int op_code, hipStream_t stream);

// out[r*cols + c] = in[r*stride0 + c*stride1]   (strides in ELEMENTS)
// LDS-staged tiles when neither axis is contiguous on the write side.
void launch_pack2d(void* out, const void* in, long long rows, long long cols,
                   long long stride0, long long stride1, int elem_size,
                   hipStream_t stream);

// in is contiguous (rows, cols); out[r*stride0 + c*stride1] = in[r*cols + c]
void launch_unpack2d(void* out, const void* in, long long rows,
                     long long cols, long long stride0, long long stride1,
                     int elem_size, hipStream_t stream);

// shallow-water step stages (shallow_water.hip)
struct SwLaunchParams {
  void *fe, *fn, *q, *ke;
  void *h, *u, *v;
  void *dnh, *dnu, *dnv;
  void *doh, *dou, *dov;
  void *h2, *u2, *v2;  // double-buffer outputs for the merged stages
  long long ny, nx;
  double dx, dy, dt, nu;
  double cor_base, cor_dj;
  double ab_a, ab_b;
  int south_open, north_open, west_open, east_open;
  int east_wall, north_wall;
  int x_wrap;  // x halos are LOCAL periodic wraps (nproc_x==1), not remote
};

// Launchable stage ids.  The values are public: profiles/ and the docs
// cite them, and models/shallow_water.py mirrors this table (SwStage
// there; docs/developers.md has the id / kernel / env-knob table).  PRE =
// derived fields fe/fn/q/ke, UPDATE = tendencies + time update, FRICTION =
// lateral friction; V4 / V2 = 4 / 2 columns per thread (float32 only).
#define SW_STAGE_LIST(X)                                                \
  X(SW_PRE_SCALAR, 1)                                                   \
  X(SW_UPDATE_SCALAR, 6)                                                \
  X(SW_FRICTION_SCALAR, 7)                                              \
  X(SW_UPDATE_MERGED_SCALAR, 8) /* PRE + UPDATE in one pass */          \
  X(SW_PRE_V4, 11)                                                      \
  X(SW_UPDATE_V4, 16)                                                   \
  X(SW_FRICTION_V4, 17)                                                 \
  X(SW_UPDATE_V4_MERGED, 18)                                            \
  X(SW_UPDATE_V2, 19)                                                   \
  X(SW_UPDATE_V2_NT, 20) /* + nontemporal streaming hints */            \
  X(SW_UPDATE_V2_TILE4, 21) /* band-tiled blocks: 4 / 8 / 16 rows */    \
  X(SW_UPDATE_V2_TILE8, 22)                                             \
  X(SW_UPDATE_V2_TILE16, 23)                                            \
  X(SW_FRICTION_V2, 27)                                                 \
  X(SW_FRICTION_V2_INTERIOR, 28) /* halo-independent pairs (overlap) */ \
  X(SW_FRICTION_V2_RING, 29)     /* the rest of SW_FRICTION_V2 */       \
  X(SW_STEP1, 30) /* whole world-1 step, one launch */                  \
  X(SW_STEP1_512, 31)                                                   \
  X(SW_FUSED_FAST_RINGA, 32) /* LDS-fused update+friction + ring A */   \
  X(SW_FUSED_RINGB, 33)      /* ring friction from the u'/v' strip */   \
  X(SW_FUSED_RING3, 34)      /* 32 + 33 back to back (world 1) */

enum SwStage : int {
#define SW_STAGE_ENUM(name, value) name = value,
  SW_STAGE_LIST(SW_STAGE_ENUM)
#undef SW_STAGE_ENUM
};

enum SwStageStatus : int {
  SW_STAGE_OK = 0,
  SW_STAGE_UNKNOWN = 1,   // not a SwStage id: nothing launched
  SW_STAGE_F32_ONLY = 2,  // float-only stage with f64 buffers: ditto
};

SwStageStatus launch_sw_stage(int stage, const SwLaunchParams& p,
                              int is_double, hipStream_t stream);

// shallow-water model halo-exchange helpers (halo.hip): periodic wrap and
// multi-field column pack/unpack (up to 3 fields)
void launch_halo_wrap(void* const* fields, int nf, long long ny,
                      long long nx, int side, int is_double,
                      hipStream_t stream);
void launch_pack_cols(void* buf, void* const* fields, int nf, long long ny,
                      long long nx, long long col, int is_double,
                      hipStream_t stream);
void launch_unpack_cols(void* const* fields, const void* buf, int nf,
                        long long ny, long long nx, long long col,
                        int is_double, hipStream_t stream);

// corner pack/unpack for the single-group halo exchange (halo.hip)
void launch_pack_corners(void* buf, void* const* fields, int nf,
                         long long ny, long long nx, int is_double,
                         hipStream_t stream);
void launch_unpack_corners(void* const* fields, const void* buf, int nf,
                           long long ny, long long nx, int mask,
                           int is_double, hipStream_t stream);

// merged halo staging (halo.hip): one launch covering the periodic wrap,
// both column packs and the corner pack (resp. the column + corner
// unpacks) — the
// per-exchange launch count is what bounds strong scaling once the local
// domain is small.  Null buffer => that segment is skipped; wrap_side -1
// => no wrap.  The unpack skips a column's j=0 / j=ny-1 cell when the
// corner segment of the SAME launch writes it (cor_mask bit set), which
// preserves the "corners win" ordering rule of parallel/grid.halo_plan.
void launch_pack_halo(void* const* fields, int nf, long long ny,
                      long long nx, int wrap_side, void* cb0, long long c0,
                      void* cb1, long long c1, void* cor, int is_double,
                      hipStream_t stream);
void launch_unpack_halo(void* const* fields, int nf, long long ny,
                        long long nx, void* cb0, long long c0, void* cb1,
                        long long c1, void* cor, int cor_mask,
                        int is_double, hipStream_t stream);

// N-d halo staging for parallel/halo.HaloExchanger (halo.hip).  One launch
// moves up to kHaloDirs segments; each segment is a (h, wd) window of
// every level of every field, laid out [field][level][row][col] in its
// staging slot.  Segments are compacted to the front; unused ones carry
// end == total.  skip_lo / skip_hi (a plain pack ignores them) make a
// full-height column strip leave its first / last `w` rows to a corner
// segment of the same launch.  Staging indices are 32-bit (total < 2^31,
// checked by the caller); offsets into a field are 64-bit.
constexpr int kHaloMaxFields = 8;
constexpr int kHaloDirs = 8;

struct HaloNdSeg {
  void* buf;             // this segment's staging slot
  long long y0, x0;      // window origin inside a (ny, nx) level
  unsigned h, wd;        // window size
  unsigned start, end;   // work-item range [start, end) of this segment
  int skip_lo, skip_hi;
};

struct HaloNdArgs {
  void* f[kHaloMaxFields];
  HaloNdSeg seg[kHaloDirs];
  long long ny, nx;
  unsigned levels, total;
  int nf, w;
};

// unpack == 0: staging <- fields; unpack == 1: fields <- staging;
// unpack == 2: the adjoint's pack — staging <- fields, except that the
// skip_lo / skip_hi rows store a zero word (the forward unpack never wrote
// those cells from this slot, so no gradient flows back through them).
// elem_size must be 1, 2, 4 or 8.
void launch_halo_nd(const HaloNdArgs& a, int unpack, int elem_size,
                    hipStream_t stream);

// Accumulate step of the halo exchange's adjoint (halo.hip).  One work
// item per cell of the 2*w-thick frame (halo_geom.h: halo_frame) of every
// level of every field.  The item starts from its own cell — or from 0
// when the cell lies in a receive window with `zero` set, because the
// forward exchange overwrote it — and adds, from the last entry to the
// first, the staging element of every entry with `acc` set whose send
// window holds the cell.
// float16 / bfloat16 sum in float32 and round once at the store.  Work and
// staging indices are 32-bit (total < 2^31, checked by the caller);
// offsets into a field are 64-bit.
struct HaloAdjSeg {
  const void* buf;  // received slot of this entry, [field][level][row][col]
  int sy, sx;       // send-window origin: where the terms are added
  int ry, rx;       // receive-window origin: what is zeroed
  unsigned h, wd;   // window size
  int acc, zero;
};

struct HaloAdjArgs {
  void* f[kHaloMaxFields];
  HaloAdjSeg seg[kHaloDirs];
  long long ny, nx;
  unsigned levels, total;    // total = nf * levels * per_level
  unsigned per_level, band;  // see HaloFrame
  int nf, w, full;
};

// dt_code must be DT_F32, DT_F64, DT_F16 or DT_BF16.
void launch_halo_adjoint_acc(const HaloAdjArgs& a, int dt_code,
                             hipStream_t stream);

// Fused halo stencil of parallel/stencil.HaloStencil (stencil.hip).  One
// launch covers every (ny, nx) plane of every field.  A workgroup owns a
// kStencilTileY x kStencilTileX tile of output cells of one plane: it
// fills an LDS tile with a `w`-cell apron, converted to the accumulate
// type (float32 for f16 / bf16 / f32, float64 for f64), then every thread
// sums the taps, in the order given and from 0, for its outputs.
//
// mode 0 (apply): the outputs are the interior cells; an input cell of the
// halo is read through the 3 x 3 region table, indexed
// [low halo, interior, high halo] along y times the same along x: the
// cell's own value, the input field at an offset (a local periodic wrap),
// or a receive staging slot laid out [field][level][row][col].  Only the
// interior of `out` is written.
// mode 1 (transposed): the outputs are all cells; an input cell counts
// only where it is interior and reads as 0 elsewhere; the region table is
// not used.  `tap_off` then carries the negated offsets.
//
// Block index, plane index and tile indices are 32-bit.  A launch holds
// fewer than 2^32 threads, so the caller checks blocks < 2^32 /
// kStencilBlock = 2^24; offsets into a field or a slot are 64-bit.
constexpr int kStencilMaxTaps = 81;
constexpr int kStencilMaxWidth = 4;
constexpr int kStencilTileX = 64;
constexpr int kStencilTileY = 32;
constexpr int kStencilBlock = 256;  // threads per block

enum StencilSource : int {
  STENCIL_OWN = 0,     // the cell itself
  STENCIL_OFFSET = 1,  // the input field at (y + dj, x + di)
  STENCIL_SLOT = 2,    // staging slot element (y - ry, x - rx)
};

struct StencilRegion {
  const void* buf;  // STENCIL_SLOT: the slot
  long long shift;  // STENCIL_OFFSET: dj * nx + di
  int kind;
  int ry, rx;       // STENCIL_SLOT: origin of the slot's window
  unsigned h, wd;   // STENCIL_SLOT: extent of the slot's window
};

struct HaloStencilArgs {
  const void* in[kHaloMaxFields];
  void* out[kHaloMaxFields];
  StencilRegion reg[9];
  union {  // coefficients in the accumulate type
    double f64[kStencilMaxTaps];
    float f32[kStencilMaxTaps];
  } coef;
  int tap_off[kStencilMaxTaps];  // dy * (kStencilTileX + 2 * w) + dx
  long long ny, nx;
  unsigned levels, tiles_y, tiles_x;
  int w, ntaps;
  double* partials;  // launch_halo_stencil_dot: one slot per block
};

// dt_code must be DT_F32, DT_F64, DT_F16 or DT_BF16; `blocks` is
// nf * levels * tiles_y * tiles_x.  Returns the launch's status.
hipError_t launch_halo_stencil(const HaloStencilArgs& a, int mode,
                               int dt_code, unsigned blocks,
                               hipStream_t stream);

// Mode 0 of the same kernel with its DOT epilogue: block `b` also writes
// a.partials[b], its part of in . out over the interior (krylov.hip has
// the definition of that sum and its order).  The stored outputs are those
// of launch_halo_stencil, bit for bit.
hipError_t launch_halo_stencil_dot(const HaloStencilArgs& a, int dt_code,
                                   unsigned blocks, hipStream_t stream);

// Mode 0 of the same kernel with its CHEB epilogue: one Chebyshev
// iteration (parallel/chebyshev.StencilChebyshev) in one launch.  `in` is
// the current direction d and `out` the next one, a different buffer
// because other blocks read this block's cells of d as their apron.  With
// q = A d from the tap loop, per interior cell and in the accumulate type,
// in this order:
//   xn = x + d;  rn = r - q;  dn = c1 * d + c2 * rn
// xn and rn are stored in place, dn to `out`.  Only interior cells of x,
// r and out are written; c1 and c2 are rounded once to the accumulate
// type.  float32 and float64 only.
struct HaloChebArgs : HaloStencilArgs {
  void* x[kHaloMaxFields];
  void* r[kHaloMaxFields];
  double c1, c2;
};

static_assert(sizeof(HaloChebArgs) < 4096,
              "the kernel arguments must stay under 4 KiB");

// dt_code must be DT_F32 or DT_F64 (anything else launches nothing; the
// caller checks).
hipError_t launch_halo_stencil_cheb(const HaloChebArgs& a, int dt_code,
                                    unsigned blocks, hipStream_t stream);

// Krylov layer over HaloStencil (krylov.hip; parallel/cg.StencilCG).
//
// The elementwise kernels run on the tile grid of the stencil's mode 0: a
// 256-thread block owns a kStencilTileY x kStencilTileX tile of interior
// cells of one (ny, nx) plane, `blocks` = nf * levels * tiles_y * tiles_x
// < 2^24, block index 32-bit, offsets 64-bit.  Only interior cells
// (w <= y < ny - w, w <= x < nx - w) are read or written.
//
// An inner product is the sum over the interior cells of
// double(a[c]) * double(b[c]), accumulated in float64 in one fixed order
// (next to krylov_block_sum in krylov_reduce.h); block `b` writes
// partials[b] and launch_krylov_finish adds the partials into one double.
struct KrylovArgs {
  const void* a[kHaloMaxFields];  // dot: a;  update: p;  direction: r
  const void* b[kHaloMaxFields];  // dot: b;  update: q
  void* x[kHaloMaxFields];        // update: x
  void* r[kHaloMaxFields];        // update: r;  direction: p
  const double* num;              // alpha or beta = *num / *den, 0 when
  const double* den;              // *den == 0
  double* partials;               // dot, update
  long long ny, nx;
  unsigned levels, tiles_y, tiles_x;
  int w;
};

enum KrylovOp : int {
  KRYLOV_DOT = 0,        // partials of a . b
  KRYLOV_UPDATE = 1,     // x += alpha p, r -= alpha q, partials of r . r
  KRYLOV_DIRECTION = 2,  // p = r + beta p
};

// KRYLOV_DOT takes the four stencil dtypes, the other two DT_F32 and
// DT_F64 only (anything else launches nothing; the caller checks).
hipError_t launch_krylov(const KrylovArgs& a, int op, int dt_code,
                         unsigned blocks, hipStream_t stream);

// One block: result[0] = sum of partials[0, n) in the fixed order;
// `save`, when not null, first receives the old result[0].
hipError_t launch_krylov_finish(const double* partials, unsigned n,
                                double* result, double* save,
                                hipStream_t stream);
