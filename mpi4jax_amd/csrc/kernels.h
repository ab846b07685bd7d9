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
  // SW_STEP1 / SW_STEP1_512: the most fast tiles of one tile column that a
  // block marches through; 0 = the launcher's default
  int march;
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

// Variable-coefficient halo stencil of
// parallel/varstencil.VariableHaloStencil (varstencil.hip).  The taps are
// ntaps <= kVarStencilMaxTaps offsets (dy, dx), |dy|, |dx| <= w, and `coef`
// holds one (ny, nx) plane of the accumulate type per tap, shared by every
// level of every field; only its interior cells are read.
//
// A workgroup owns one (4 * rows) x kStencilTileX tile of output cells for
// levels [chunk * lpb, min(levels, (chunk + 1) * lpb)) of one field, with
// rows = kVarStencilRowsF32 for float accumulation and kVarStencilRowsF64
// for double; tiles_y counts tiles of that height.  A thread keeps the
// coefficients of its outputs in registers for the whole march.  The block
// index decodes, fastest first, to (tile x, tile y, chunk, field):
// `blocks` = nf * chunks * tiles_y * tiles_x < 2^24, 32-bit; offsets into
// a field, a slot or `coef` are 64-bit.
//
// mode 0 (apply): out[l, j, i] = sum_t K_t[j, i] * v[l, j + dy_t, i + dx_t]
// on interior cells, halo cells of v read through the region table as in
// HaloStencilArgs; the sum is formed from 0 in tap order.
// mode 1 (transposed): every cell p is written with the sum, in the same
// order, of K_t[p - o_t] * in[p - o_t] over the taps whose source cell
// p - o_t is interior; the region table is not used.
// mode 2: mode 0, and block `b` also writes partials[b], its part of
// in . out over its interior cells in float64: a thread adds
// double(in) * double(out as stored) level by level and row by row, then
// krylov_block_sum.  The stored outputs are those of mode 0, bit for bit.
constexpr int kVarStencilMaxTaps = 13;
constexpr int kVarStencilRowsF32 = 8;
constexpr int kVarStencilRowsF64 = 4;

struct HaloVarStencilArgs {
  const void* in[kHaloMaxFields];
  void* out[kHaloMaxFields];
  StencilRegion reg[9];
  const void* coef;  // (ntaps, ny, nx) in the accumulate type
  int tap_dy[kVarStencilMaxTaps];
  int tap_dx[kVarStencilMaxTaps];
  long long ny, nx;
  unsigned levels, lpb, chunks, tiles_y, tiles_x;
  int w, ntaps;
  double* partials;  // mode 2: one slot per block
};

// dt_code must be DT_F32, DT_F64, DT_F16 or DT_BF16.  Returns the launch's
// status.
hipError_t launch_halo_varstencil(const HaloVarStencilArgs& a, int mode,
                                  int dt_code, unsigned blocks,
                                  hipStream_t stream);

// 3-D halo stencil of parallel/stencil3d.HaloStencil3D (stencil3d.hip).
// A field is `columns` independent (nz, ny, nx) columns, levels = columns *
// nz planes in the exchanger's layout; z is local and has no halo.  The
// taps are ntaps <= kStencil3dMaxTaps triples (dz, dy, dx), |dz| <= rz <= 2,
// |dy|, |dx| <= w, sorted by dz (tap_begin[j] is the first tap of
// dz = j - rz, tap_begin[2 rz + 1] = ntaps) and in the order they are added
// inside one dz; `tap_off` is dy * (kStencilTileX + 2 * w) + dx, negated
// for mode 1.
//
// A workgroup owns one kStencilTileY x kStencilTileX tile of one column for
// the output planes [chunk * zc, min(nz, (chunk + 1) * zc)) and marches
// along z with one input plane resident in LDS (double-buffered) and
// 2 rz + 1 output planes in registers.  The block index decodes, fastest
// first, to (tile x, tile y, chunk, column, field): `blocks` = nf * columns
// * chunks * tiles_y * tiles_x < 2^24, 32-bit; offsets into a field or a
// slot are 64-bit.
//
// A source plane outside [0, nz) is taken modulo nz when periodic_z is set
// (the caller checks nz >= 2 rz + 1); otherwise its taps are not formed.
//
// mode 0 (apply): out[b, k, j, i] = sum_t K_t * v[b, k + dz_t, j + dy_t,
// i + dx_t] on interior (j, i), halo cells of v read through the region
// table as in HaloStencilArgs; the sum is formed from 0 in tap order.
// mode 1 (transposed): every cell p of every plane k is written with the
// sum, in the same order, of K_t * in[b, k - dz_t, p - (dy_t, dx_t)] over
// the taps whose source cell is interior; the region table is not used.
// mode 2: mode 0, and block `b` also writes partials[b], its part of
// in . out over its interior cells in float64: a thread adds
// double(in) * double(out as stored) plane by plane from z0 upward and row
// by row, then krylov_block_sum.  The stored outputs are those of mode 0,
// bit for bit.
constexpr int kStencil3dMaxTaps = 32;
constexpr int kStencil3dMaxRz = 2;

struct HaloStencil3dArgs {
  const void* in[kHaloMaxFields];
  void* out[kHaloMaxFields];
  StencilRegion reg[9];
  union {  // coefficients in the accumulate type
    double f64[kStencil3dMaxTaps];
    float f32[kStencil3dMaxTaps];
  } coef;
  int tap_off[kStencil3dMaxTaps];
  int tap_begin[2 * kStencil3dMaxRz + 2];
  long long ny, nx;
  unsigned levels, nz, columns, zc, chunks, tiles_y, tiles_x;
  int w, rz, ntaps, periodic_z;
  double* partials;  // mode 2: one slot per block
};

// dt_code must be DT_F32, DT_F64, DT_F16 or DT_BF16, a.rz in 0..2.  Returns
// the launch's status.
hipError_t launch_halo_stencil3d(const HaloStencil3dArgs& a, int mode,
                                 int dt_code, unsigned blocks,
                                 hipStream_t stream);

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

// Vertical line solves of parallel/zline.ZLineSolver (zline.hip).  T is the
// tridiagonal matrix along z of a 3-D stencil's taps (dz, 0, 0): a below
// the diagonal, b on it, c above, the same for every column; under
// periodic z it also has a in its top right and c in its bottom left
// corner.  A field is `columns` (nz, ny, nx) columns as in
// HaloStencil3dArgs.
//
// `tables` is (4, nz) in the field dtype, from the host's float64 Thomas
// factorisation rounded once:
//   row 0  inv_k = 1 / (b_k - a cp_{k-1})            the pivots' reciprocals
//   row 1  cp_k  = c inv_k
//   row 2  qs_k: periodic only, q = T'^{-1} u over (1 + q_0 + g q_{nz-1})
//   row 3  lo_k  = a for k >= 1; lo_0 = g = a / gamma (0 when not periodic)
// where periodic z factors the Sherman-Morrison matrix T' (gamma = -b,
// b_0' = b - gamma, b_{nz-1}' = b - a c / gamma, u = (gamma, 0, .., 0, c)).
//
// A thread owns one interior (j, i) column of one field and marches over
// z; a 256-thread block owns kZlineTileY x kZlineTileX columns, lanes
// along x.  The block index decodes, fastest first, to (tile x, tile y,
// column, field): `blocks` = nf * columns * tiles_y * tiles_x < 2^24,
// 32-bit; offsets into a field are 64-bit.  Per thread:
//   forward, k = 0 .. nz-1:  y_0 = r_0 inv_0,
//                            y_k = (r_k - lo_k y_{k-1}) inv_k
//   back, k = nz-1 .. 0:     s_{nz-1} = y_{nz-1},  s_k = y_k - cp_k s_{k+1}
//   periodic, k = 0 .. nz-1: z_k = s_k - qs_k (s_0 + lo_0 s_{nz-1});
//   otherwise z_k = s_k, stored in the back sweep.
// y_k (then s_k under periodic z) of the planes k < lds_planes is kept in
// lds_planes * 256 * sizeof(dtype) bytes of dynamic LDS, of the other
// planes in z[k] itself.  Only interior cells of z are written; z aliases
// no other field.
//
// ZLINE_SOLVE: z = T^{-1} r.
// ZLINE_PCG_UPDATE: the forward sweep first forms, per plane, exactly
// KRYLOV_UPDATE's x + alpha p and rn = r - alpha q (alpha = *num / *den
// as there), stores both, adds double(rn) * double(rn) to the thread's
// first sum, and eliminates on rn.  The sweep that stores z_k re-reads the
// stored rn and adds double(rn) * double(z_k) to the thread's second sum
// (k descending, or ascending under periodic z).  Each sum goes through
// krylov_block_sum; block `b` writes partials[b] = its r . r and
// partials[blocks + b] = its r . z.
constexpr int kZlineTileX = 64;
constexpr int kZlineTileY = 4;
constexpr int kZlineBlock = 256;
// Dynamic LDS a block may ask for: 64 KiB less the reduction's slots.
constexpr int kZlineMaxLds = 65536 - 64;

enum ZLineMode : int {
  ZLINE_SOLVE = 0,
  ZLINE_PCG_UPDATE = 1,
};

struct ZLineArgs {
  const void* p[kHaloMaxFields];  // update only
  const void* q[kHaloMaxFields];  // update only
  void* x[kHaloMaxFields];        // update only
  void* r[kHaloMaxFields];        // solve: read;  update: read and written
  void* z[kHaloMaxFields];
  const void* tables;
  const double* num;  // update: alpha = *num / *den, 0 when *den == 0
  const double* den;
  double* partials;   // update: 2 * blocks slots
  long long ny, nx;
  unsigned nz, columns, tiles_y, tiles_x, lds_planes;
  int w, periodic;
};

// dt_code must be DT_F32 or DT_F64 (anything else launches nothing; the
// caller checks), lds_planes <= nz and lds_planes * 256 * sizeof(dtype) <=
// kZlineMaxLds.  Returns the launch's status.
hipError_t launch_zline(const ZLineArgs& a, int mode, int dt_code,
                        unsigned blocks, hipStream_t stream);

// The same line solves by parallel cyclic reduction (zline_pcr.hip;
// ZLineSolver with method="pcr"), for tall columns on planes too small to
// fill the GPU with one thread per column.  T, the fields and the two
// modes are those of ZLineArgs.
//
// `tables` is (2 L + 2, nz) in the field dtype, L = `levels` =
// ceil(log2 nz), from the host's float64 reduction of T (of the
// Sherman-Morrison matrix T' under periodic z) rounded once.  With lo, d,
// up the rows of the matrix, lo_0 = up_{nz-1} = 0, level l has stride
// s = 2^l and
//   row l      alpha_k = -lo_k / d_{k-s}   (0 where k - s < 0)
//   row L + l  gamma_k = -up_k / d_{k+s}   (0 where k + s >= nz)
// and leaves lo'_k = alpha_k lo_{k-s}, up'_k = gamma_k up_{k+s},
// d'_k = d_k + alpha_k up_{k-s} + gamma_k lo_{k+s} to the next level;
//   row 2 L      inv_k = 1 / d_k after the last level
//   row 2 L + 1  qs_k as in ZLineArgs (periodic only)
// and tables[0][0], which no level reads, holds g under periodic z.
//
// A 256-thread block owns C = `cols` (8, 16, 32 or 64) consecutive interior
// cells of one row of one column of one field: lane = t % C along x, and
// thread t works on the planes k = t / C, t / C + 256 / C, ...  The block
// index decodes, fastest first, to (tile x, row, column, field): `blocks` =
// nf * columns * rows * tiles_x < 2^24, 32-bit; offsets into a field are
// 64-bit.  Two buffers of nz * C values, [k][lane], live in
// 2 * nz * C * sizeof(dtype) <= kZlineMaxLds bytes of dynamic LDS.  Per
// cell:
//   v_k = r_k;  per level  v'_k = v_k + alpha_k v_{k-s} + gamma_k v_{k+s},
//   a neighbour outside 0..nz-1 neither read nor multiplied;
//   s_k = v_k inv_k;  z_k = s_k, or under periodic z
//   z_k = s_k - qs_k (s_0 + g s_{nz-1}).
// The arithmetic of a cell does not depend on C.  Cells past the ragged
// end of a row are neither read nor written.
//
// ZLINE_PCG_UPDATE: the load forms x + alpha p and rn = r - alpha q as
// ZLineArgs says, stores both, adds double(rn)^2 to the thread's first sum
// and reduces rn; the store re-reads the thread's own rn and adds
// double(rn) * double(z_k) to its second sum.  A thread adds in ascending
// k; then krylov_block_sum twice, into partials[b] and
// partials[blocks + b].
struct ZLinePcrArgs {
  const void* p[kHaloMaxFields];  // update only
  const void* q[kHaloMaxFields];  // update only
  void* x[kHaloMaxFields];        // update only
  void* r[kHaloMaxFields];        // solve: read;  update: read and written
  void* z[kHaloMaxFields];
  const void* tables;
  const double* num;  // update: alpha = *num / *den, 0 when *den == 0
  const double* den;
  double* partials;   // update: 2 * blocks slots
  long long ny, nx;
  unsigned nz, columns, rows, tiles_x, levels, cols_log2;
  int w, periodic;
};

// dt_code must be DT_F32 or DT_F64 (anything else launches nothing; the
// caller checks), cols_log2 in 3..6, levels = ceil(log2 nz), nz >= 3 when
// periodic, and the two buffers within kZlineMaxLds.  Returns the
// launch's status.
hipError_t launch_zline_pcr(const ZLinePcrArgs& a, int mode, int dt_code,
                            unsigned blocks, hipStream_t stream);

// Per-column tridiagonal solves of parallel/ztridiag.ColumnTridiagonal
// (ztridiag.hip).  Every interior (j, i) has a system of its own along z:
// row k is l_k x_{k-1} + d_k x_k + u_k x_{k+1} with the bands `lower`,
// `diag`, `upper`, three contiguous (nz, ny, nx) tensors of one dtype
// (band_code: DT_F32 or DT_F64); l_0 and u_{nz-1} are never used and z is
// closed.  Only interior cells of any tensor are read or written.
//
// The factorisation runs in float64 whatever the dtypes:
//   pivot_0 = d_0,  pivot_k = d_k - l_k cp_{k-1},
//   inv_k = 1 / pivot_k,  cp_k = u_k inv_k
// and inv, cp and lo = l are rounded once to the field dtype.  `factors`
// is (3, nz, ny, nx) in the field dtype, in the order inv, cp, lo.
//
// A right-hand side is one (field, batch column) pair, entry s = field *
// batch + column of nrhs = nf * batch; a field is `batch` (nz, ny, nx)
// columns.  A thread owns one interior (j, i) and carries R =
// rhs_per_thread (1, 2 or 4) consecutive entries through one march over z;
// a 256-thread block owns kZlineTileY x kZlineTileX cells, lanes along x.
// The block index decodes, fastest first, to (tile x, tile y, group of R
// entries): `blocks` = ceil(nrhs / R) * tiles_y * tiles_x < 2^24, 32-bit;
// offsets into a tensor are 64-bit.  Per entry, in the field dtype:
//   forward, k = 0 .. nz-1:  y_0 = r_0 inv_0,
//                            y_k = (r_k - lo_k y_{k-1}) inv_k
//   back, k = nz-1 .. 0:     x_{nz-1} = y_{nz-1},  x_k = y_k - cp_k x_{k+1}
// and what an entry computes does not depend on R.  Entries past nrhs in
// the last group are not touched.
//
// ZTRIDIAG_FACTOR: bands -> factors, one thread per cell, blocks = tiles_y
// * tiles_x.  Block b also stores status[2 b] = the smallest pivot its
// columns saw, a pivot that is not finite counting as -inf and a column
// counting up to and including its first pivot that is not positive, and
// status[2 b + 1] = that pivot's plane (the lower plane on a tie).  Every
// tile holds an interior column.  Plain stores, no atomics.
// ZTRIDIAG_SOLVE: x = T^{-1} r from `factors`.  y_k of the planes
// k < lds_planes lives in dynamic LDS, slot (k * R + j) * 256 + thread for
// entry j of the group, of the planes above in x[k] itself:
// lds_planes * R * 256 * sizeof(dtype) <= kZlineMaxLds.
// ZTRIDIAG_SOLVE_BANDS: the same from the bands, factorised on the way up
// by the same float64 recurrence and rounded the same way, so the result
// is that of FACTOR + SOLVE bit for bit; no pivot is looked at.  The
// stash has R + 1 slots per plane, the last for cp_k: lds_planes *
// (R + 1) * 256 * sizeof(dtype) <= kZlineMaxLds; cp_k of the planes above
// goes to `work`, (groups, nz - lds_planes, ny, nx) in the field dtype.
// x aliases no other tensor.
enum ZTridiagOp : int {
  ZTRIDIAG_FACTOR = 0,
  ZTRIDIAG_SOLVE = 1,
  ZTRIDIAG_SOLVE_BANDS = 2,
};

struct ZTridiagArgs {
  const void* r[kHaloMaxFields];  // solves
  void* x[kHaloMaxFields];        // solves
  const void* lower;              // FACTOR, SOLVE_BANDS
  const void* diag;
  const void* upper;
  void* factors;   // FACTOR: written;  SOLVE: read
  void* work;      // SOLVE_BANDS with lds_planes < nz
  double* status;  // FACTOR: two slots per block
  long long ny, nx;
  unsigned nz, batch, nrhs, tiles_y, tiles_x, lds_planes;
  int w;
};

// dt_code must be DT_F32 or DT_F64, and so must band_code unless op is
// ZTRIDIAG_SOLVE (anything else launches nothing; the caller checks);
// rhs_per_thread 1, 2 or 4 for the solves.  Returns the launch's status.
hipError_t launch_ztridiag(const ZTridiagArgs& a, int op, int dt_code,
                           int band_code, int rhs_per_thread,
                           unsigned blocks, hipStream_t stream);
