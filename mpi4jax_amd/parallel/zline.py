"""Vertical line solves for :class:`~.stencil3d.HaloStencil3D`.

``T`` is the tridiagonal matrix along z made of the stencil's taps at
``(dz, 0, 0)``: ``a`` (``dz = -1``), ``b`` (centre) and ``c`` (``dz = +1``),
the same for every column.  Under ``z_boundary="zero"`` it is plain
tridiagonal; under ``"periodic"`` it also has ``a`` in its top right and
``c`` in its bottom left corner.  A :class:`ZLineSolver` (built by
``HaloStencil3D.make_line_solver``) computes ``z = T^{-1} r`` on every
interior column.  z is never decomposed and stores no halo, so a line solve
needs no communication; it is the preconditioner of
:class:`~.pcg.StencilPCG`.

Tables.  ``T`` does not vary by column, so its Thomas factorisation is done
once, on the host, in float64 and rounded once to ``Acc``:
``inv_k = 1 / (b_k - a cp_{k-1})`` and ``cp_k = c inv_k``.  A pivot that is
not positive and finite raises ``ValueError``.  Periodic z factors the
Sherman-Morrison matrix ``T'`` (``gamma = -b``, ``b_0' = b - gamma``,
``b_{nz-1}' = b - a c / gamma``) and adds ``qs = q / (1 + q_0 + g q_{nz-1})``
with ``q = T'^{-1} (gamma, 0, .., 0, c)`` and ``g = a / gamma``.  With
``a = c = 0`` both boundaries degenerate to a scaling by ``1 / b``.  A
periodic ``T`` is refused as singular when that denominator does not rise
above the rounding noise of its own three terms, ``1024 nz eps64 (1 + |q_0|
+ |g q_{nz-1}|)``: for ``b = -(a + c)`` it is 0 in real arithmetic, and in
float64 anything from 0 to ``eps64``.  The executors only multiply:

* forward, ``k`` up: ``y_0 = r_0 inv_0``, ``y_k = (r_k - a y_{k-1}) inv_k``;
* back, ``k`` down: ``s_{nz-1} = y_{nz-1}``, ``s_k = y_k - cp_k s_{k+1}``;
* periodic only: ``z_k = s_k - qs_k (s_0 + g s_{nz-1})``; otherwise
  ``z = s``.

Executors: the native one (``csrc/zline.hip``) gives every interior
``(j, i)`` column to one thread that marches over z.  It keeps ``y`` of the
first ``lds_planes`` planes in LDS and of the planes above in ``z`` itself.
The Python executor (CPU, or ``MPI4JAX_AMD_HALO_PY=1``) runs the same
recurrences on the same tables by slicing over planes.  The native kernel
contracts multiply and add, so the two differ by rounding except where
every product is exact.

The march is serial in z: its parallelism is the number of columns,
``nfields * B * ny * nx``.  Very tall columns on very small horizontal
grids leave the GPU few threads.

``method="pcr"`` is for those: parallel cyclic reduction.  With ``lo``,
``d``, ``up`` the rows of ``T`` (of ``T'`` under periodic z) and stride
``s = 1, 2, 4, ...``, a level adds ``alpha_k = -lo_k / d_{k-s}`` times row
``k - s`` and ``gamma_k = -up_k / d_{k+s}`` times row ``k + s`` to row
``k``, which moves its off-diagonals out to distance ``2 s``:
``lo'_k = alpha_k lo_{k-s}``, ``up'_k = gamma_k up_{k+s}``,
``d'_k = d_k + alpha_k up_{k-s} + gamma_k lo_{k+s}``.  After ``levels =
ceil(log2 nz)`` levels the matrix is diagonal.  ``T`` is the same for
every column, so the host runs this once in float64 (``_pcr``, after
``_thomas`` for its refusals, ``qs`` and ``g``; a ``d`` that is not
positive and finite is refused in the same words) and rounds once; the
executors only multiply:

* per level: ``v'_k = v_k + alpha_k v_{k-s} + gamma_k v_{k+s}``, a
  neighbour outside ``0..nz-1`` neither read nor multiplied;
* ``s_k = v_k inv_k`` with ``inv_k = 1 / d_k`` of the last level, then the
  periodic correction above.

The native executor (``csrc/zline_pcr.hip``) gives ``columns_per_block``
cells of one row, with all their planes, to a block that keeps two ``nz x
columns_per_block`` buffers in LDS; the host takes the widest of 64, 32,
16 and 8 that fits in LDS, and no wider than covers an interior row.  The
Python executor slices over planes.  ``nz`` is limited to what fits at 8
columns: 1023 in float32, 511 in float64.

float32 and float64 only.
"""

import math
import sys

import torch

from .cg import CG_DTYPES

BLOCK = 256            # kZlineBlock of csrc/kernels.h
TILE_Y, TILE_X = 4, 64  # kZlineTileY, kZlineTileX
MAX_LDS = 65536 - 64   # kZlineMaxLds: 64 KiB less the reduction's slots
PCR_COLUMNS = (8, 16, 32, 64)  # tile widths of csrc/zline_pcr.hip
# A periodic T counts as singular when its Sherman-Morrison denominator is
# within this many nz * eps64 of the terms it sums (see _thomas).  Over nz in
# 3..70 the singular bands (-1, 2, -1) give at most 0.09 of these units and
# the nearly singular (-1, 2 + 1e-6, -1) 5e8.
_SINGULAR = 1024.0


def _not_definite(k, pivot):
    return ValueError(
        f"the stencil is not positive definite along z: pivot {k} of "
        f"its vertical tridiagonal part is {pivot}")


def _thomas(nz, a, b, c, periodic):
    """The four table rows as float64 lists: inv, cp, qs, lo.

    Raises ``ValueError`` for a pivot that is not positive and finite, and
    under periodic z for a Sherman-Morrison denominator ``den = 1 + q_0 +
    g q_{nz-1}`` that is not finite or not above ``_SINGULAR * nz * eps64 *
    (1 + |q_0| + |g q_{nz-1}|)``, the rounding noise of the sum itself: a
    singular periodic ``T`` (``b = -(a + c)``) has ``den = 0`` in real
    arithmetic, which float64 returns as anything from 0 to about ``eps64``
    depending on ``nz``."""
    bad = _not_definite
    diag = [b] * nz
    gamma = -b
    if periodic:
        if not (math.isfinite(b) and b > 0.0):
            raise bad(0, b)
        diag[0], diag[-1] = b - gamma, b - a * c / gamma
    inv, cp = [], []
    for k in range(nz):
        pivot = diag[k] - (a * cp[k - 1] if k else 0.0)
        if not (math.isfinite(pivot) and pivot > 0.0):
            raise bad(k, pivot)
        inv.append(1.0 / pivot)
        cp.append(c * inv[k])
    qs, lo = [0.0] * nz, [0.0] + [a] * (nz - 1)
    if periodic:
        u = [gamma] + [0.0] * (nz - 2) + [c]
        q = []
        for k in range(nz):
            q.append((u[k] - (a * q[k - 1] if k else 0.0)) * inv[k])
        for k in range(nz - 2, -1, -1):
            q[k] -= cp[k] * q[k + 1]
        g = a / gamma
        den = 1.0 + q[0] + g * q[-1]
        tiny = _SINGULAR * nz * sys.float_info.epsilon * (
            1.0 + abs(q[0]) + abs(g * q[-1]))
        if not (math.isfinite(den) and den > tiny):
            raise bad(nz, den)
        qs, lo[0] = [v / den for v in q], g
    return inv, cp, qs, lo


def _pcr(nz, a, b, c, periodic):
    """The ``2 L + 2`` rows of the cyclic-reduction table as float64 lists:
    ``L`` of alpha, ``L`` of gamma, inv and qs, ``L = ceil(log2 nz)``.

    ``_thomas`` runs first, so every refusal of the Thomas path is made
    here in the same words; ``qs`` and ``g`` are its own.  A reduced
    diagonal entry that is not positive and finite raises the same
    ``ValueError``.  Under periodic z ``alpha[0][0]``, which no level
    reads, holds ``g``."""
    _, _, qs, lo_t = _thomas(nz, a, b, c, periodic)
    d = [b] * nz
    if periodic:
        gamma = -b  # T' of _thomas
        d[0], d[-1] = b - gamma, b - a * c / gamma
    lo, up = [0.0] + [a] * (nz - 1), [c] * (nz - 1) + [0.0]
    levels = (nz - 1).bit_length()
    alphas, gammas = [], []
    for s in (1 << level for level in range(levels)):
        al = [-lo[k] / d[k - s] if k >= s else 0.0 for k in range(nz)]
        ga = [-up[k] / d[k + s] if k + s < nz else 0.0 for k in range(nz)]
        nd = [d[k] + (al[k] * up[k - s] if k >= s else 0.0)
              + (ga[k] * lo[k + s] if k + s < nz else 0.0)
              for k in range(nz)]
        for k, pivot in enumerate(nd):
            if not (math.isfinite(pivot) and pivot > 0.0):
                raise _not_definite(k, pivot)
        lo = [al[k] * lo[k - s] if k >= s else 0.0 for k in range(nz)]
        up = [ga[k] * up[k + s] if k + s < nz else 0.0 for k in range(nz)]
        d = nd
        alphas.append(al)
        gammas.append(ga)
    if periodic:
        alphas[0][0] = lo_t[0]
    return alphas + gammas + [[1.0 / v for v in d], qs]


class ZLineSolver:
    """See the module docstring.  Build with
    ``HaloStencil3D.make_line_solver``."""

    def __init__(self, stencil, _lds_planes=None, method="thomas",
                 _pcr_columns=None):
        if method not in ("thomas", "pcr"):
            raise ValueError(
                f"method must be 'thomas' or 'pcr', got {method!r}")
        if stencil.dtype not in CG_DTYPES:
            raise TypeError(
                f"line solves support float32 and float64, the stencil was "
                f"built for {stencil.dtype}")
        band = {dz: 0.0 for dz in (-2, -1, 0, 1, 2)}
        for dz, dy, dx, coef in stencil.taps:
            if dy == 0 and dx == 0:
                band[dz] = coef
        if band[-2] != 0.0 or band[2] != 0.0:
            raise ValueError(
                "the stencil has a (+-2, 0, 0) weight: the tridiagonal part "
                "of a pentadiagonal matrix need not be positive definite")
        self.stencil = stencil
        self._bands = a, b, c = band[-1], band[0], band[1]
        nz = stencil.nz
        self._periodic = (stencil.z_boundary == "periodic"
                          and (a != 0.0 or c != 0.0))
        ex = stencil.exchanger
        self._method = method
        self._partials = self._levels = self._cols = None
        rows =(_pcr if method == "pcr" else _thomas)(
            nz, a, b, c, self._periodic)
        self._tables = torch.tensor(rows, dtype=torch.float64).to(
            stencil.acc_dtype).to(ex.device)
        if method == "pcr":
            if _lds_planes is not None:
                raise ValueError(
                    "_lds_planes belongs to method='thomas': under 'pcr' "
                    "every plane lives in LDS")
            self._levels = (nz - 1).bit_length()
            self._lds_planes = nz
            self._cols = self._pick_columns(_pcr_columns)
            return
        if _pcr_columns is not None:
            raise ValueError("_pcr_columns belongs to method='pcr'")
        most = MAX_LDS // (BLOCK * ex.dtype.itemsize)
        if _lds_planes is None:
            _lds_planes = min(nz, most)
        elif (isinstance(_lds_planes, bool)
              or not isinstance(_lds_planes, int)
              or not 0 <= _lds_planes <= min(nz, most)):
            raise ValueError(
                f"_lds_planes must be an int in 0..{min(nz, most)}, got "
                f"{_lds_planes!r}")
        self._lds_planes = _lds_planes

    def _pick_columns(self, forced):
        """The tile width ``C`` of the cyclic-reduction kernel: the largest
        of ``PCR_COLUMNS`` whose two ``nz x C`` buffers fit in LDS, and no
        more than the smallest that covers an interior row."""
        st = self.stencil
        ex = st.exchanger
        per_col = 2 * st.nz * ex.dtype.itemsize
        fits = [c for c in PCR_COLUMNS if c * per_col <= MAX_LDS]
        if not fits:
            raise ValueError(
                f"method='pcr' keeps two buffers of nz x {PCR_COLUMNS[0]} "
                f"{ex.dtype} values in LDS: nz = {st.nz} exceeds the largest "
                f"nz of {MAX_LDS // (2 * PCR_COLUMNS[0] * ex.dtype.itemsize)}")
        if forced is None:
            width = ex.nx - 2 * st.width
            cover = [c for c in PCR_COLUMNS if c >= width]
            return min(fits[-1], cover[0] if cover else PCR_COLUMNS[-1])
        if (isinstance(forced, bool) or not isinstance(forced, int)
                or forced not in fits):
            raise ValueError(
                f"_pcr_columns must be one of {fits} at nz = {st.nz}, got "
                f"{forced!r}")
        return forced

    @property
    def method(self):
        """``"thomas"`` or ``"pcr"``."""
        return self._method

    @property
    def bands(self):
        """``(a, b, c)``: the weights at ``dz = -1, 0, +1``."""
        return self._bands

    @property
    def lds_planes(self):
        """Planes of the forward sweep that the native kernel keeps in
        LDS; the planes above go through the output array.  Under
        ``"pcr"`` every plane lives in LDS: ``nz``."""
        return self._lds_planes

    @property
    def levels(self):
        """The reduction's levels under ``"pcr"``, ``ceil(log2 nz)``; None
        under ``"thomas"``."""
        return self._levels

    @property
    def columns_per_block(self):
        """The cells of one row that a block of the ``"pcr"`` kernel owns;
        None under ``"thomas"``."""
        return self._cols

    @property
    def tables(self):
        """``"thomas"``: the ``(4, nz)`` device tensor of ``inv``, ``cp``,
        ``qs`` and ``lo`` in ``Acc`` (``lo[0]`` holds ``g``).  ``"pcr"``:
        the ``(2 levels + 2, nz)`` tensor of the ``alpha`` rows, the
        ``gamma`` rows, ``inv`` and ``qs`` (``alpha[0][0]`` holds ``g``
        under periodic z)."""
        return self._tables

    def solve(self, *fields, out=None):
        """``T^{-1}`` on the interior columns of ``fields``; the inputs
        are never mutated.  Results and ``out=`` as in
        ``HaloStencil.apply``: new tensors have a zero halo, and only the
        interior of ``out`` is written."""
        st = self.stencil
        st.exchanger._check(fields)
        outs = st._outputs(fields, out, zero=True)
        self._solve_into(fields, outs)
        return st._ret(outs)

    # ------------------------------------------------------------------
    def _geom(self):
        st = self.stencil
        ex = st.exchanger
        return (ex.levels, st.nz, ex.ny, ex.nx, st.width, self._tables,
                self._periodic,
                self._cols if self._method == "pcr" else self._lds_planes)

    def _partials_buf(self):
        """Two float64 slots per block of the native kernel's grid."""
        if self._partials is None:
            st = self.stencil
            ex = st.exchanger
            w = st.width
            ty, tx = ((1, self._cols) if self._method == "pcr"
                      else (TILE_Y, TILE_X))
            tiles = -(-(ex.ny - 2 * w) // ty) * -(-(ex.nx - 2 * w) // tx)
            self._partials = torch.empty(
                2 * ex.nfields * (ex.levels // st.nz) * tiles,
                dtype=torch.float64, device=ex.device)
        return self._partials

    def _solve_into(self, rs, zs):
        if self.stencil._native():
            from .._backend import rccl

            entry = ("halo_zline_pcr_solve_nd" if self._method == "pcr"
                     else "halo_zline_solve_nd")
            getattr(rccl.ext(), entry)(list(rs), list(zs), *self._geom())
        else:
            for r, z in zip(rs, zs):
                self._columns(z).copy_(self._solve_py(self._columns(r)))

    def _columns(self, t):
        """The interior of ``t`` as ``(B, nz, ny - 2w, nx - 2w)``."""
        st = self.stencil
        ex = st.exchanger
        w = st.width
        return t.view(-1, st.nz, ex.ny, ex.nx)[:, :, w:ex.ny - w,
                                               w:ex.nx - w]

    def _solve_py(self, r):
        nz = self.stencil.nz
        if self._method == "pcr":
            tab, lv = self._tables, self._levels
            v = r
            for level in range(lv):  # 2^level < nz: both slices non-empty
                s = 1 << level
                nxt = v.clone()
                nxt[:, s:] += tab[level, s:, None, None] * v[:, :nz - s]
                nxt[:, :nz - s] += (tab[lv + level, :nz - s, None, None]
                                    * v[:, s:])
                v = nxt
            v = v * tab[2 * lv, :, None, None]
            if self._periodic:
                fac = v[:, 0] + tab[0, 0] * v[:, nz - 1]
                v = v - tab[2 * lv + 1, :, None, None] * fac[:, None]
            return v
        inv, cp, qs, lo = self._tables
        y = torch.empty_like(r)
        y[:, 0] = r[:, 0] * inv[0]
        for k in range(1, nz):
            y[:, k] = (r[:, k] - lo[k] * y[:, k - 1]) * inv[k]
        for k in range(nz - 2, -1, -1):
            y[:, k] -= cp[k] * y[:, k + 1]
        if self._periodic:
            fac = y[:, 0] + lo[0] * y[:, nz - 1]
            y -= qs[:, None, None] * fac[:, None]
        return y

    def _pcg_update(self, x, r, p, q, z, rz, pq, rz_old, rr):
        """The update step of :class:`~.pcg.StencilPCG` on this rank:
        ``alpha = rz / pq``; ``x += alpha p``; ``r -= alpha q``;
        ``z = T^{-1} r``; ``rr = r . r``; ``rz_old = rz``;
        ``rz = r . z``."""
        st = self.stencil
        if st._native():
            from .._backend import rccl

            entry = ("halo_zline_pcr_update_nd" if self._method == "pcr"
                     else "halo_zline_pcg_update_nd")
            getattr(rccl.ext(), entry)(
                x, r, p, q, z, *self._geom(), rz, pq, rz_old, rr,
                self._partials_buf())
            return
        alpha = torch.where(pq == 0, torch.zeros_like(rz), rz / pq).to(
            st.acc_dtype)
        sum_rr = sum_rz = 0.0
        for fx, fr, fp, fq, fz in zip(x, r, p, q, z):
            st._interior(fx).add_(alpha * st._interior(fp))
            ri = self._columns(fr)
            ri.sub_(alpha * self._columns(fq))
            zi = self._columns(fz)
            zi.copy_(self._solve_py(ri))
            sum_rr = sum_rr + (ri.double() * ri.double()).sum()
            sum_rz = sum_rz + (ri.double() * zi.double()).sum()
        rz_old.copy_(rz)
        rz.copy_(sum_rz)
        rr.copy_(sum_rr)
