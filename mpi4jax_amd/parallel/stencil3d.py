"""3-D halo stencil: a constant-coefficient stencil that couples the
levels of a column, on a slab decomposed in ``(y, x)`` and local in z.

A :class:`HaloStencil3D` (built by ``CartesianGrid.make_stencil3d``) takes a
shape ``(..., nz, ny, nx)`` and a real ``(2 rz + 1, 2 r + 1, 2 r + 1)``
table of weights, ``0 <= rz <= 2`` and ``1 <= r <= 4``.  Entry
``[a][b][c]`` multiplies the cell at offset ``(a - rz, b - r, c - r)`` in
``(z, y, x)``.  The third axis from the end is z: it is not decomposed and
stores no halo.  The axes before it form ``B`` independent columns, and the
exchanger sees the shape unchanged (``levels = B * nz``), with halo width
``r``.  Zero weights are dropped at build time; at most 32 taps remain.
With ``E`` and ``P_int`` exactly as in :mod:`.stencil`:

* ``apply``: ``out[b, k, j, i] = sum_t K_t * v[b, k + dz_t, j + dy_t,
  i + dx_t]`` on interior ``(j, i)`` and every ``k``, ``v = E(fields)``.
  The sum is formed in ``Acc`` from 0 in row-major table order and rounded
  once at a 16-bit store;
* ``adjoint`` is ``E^T . S^T . P_int``: every cell ``p`` of every plane
  ``k`` gets the sum, in the same order and from 0, of
  ``K_t * gout[b, k - dz_t, p - (dy_t, dx_t)]`` over the taps whose source
  cell is interior and whose source plane exists; ``ex.adjoint_`` then runs
  in place;
* ``apply_ad``, ``dot``, ``apply_dot`` and ``make_cg()`` are inherited
  from :class:`~.stencil.HaloStencil`;
* ``make_line_solver`` solves with the tridiagonal part of ``A`` along z
  (:mod:`.zline`), and ``make_cg("zline")`` uses that as the
  preconditioner of conjugate gradients (:mod:`.pcg`).

``z_boundary="zero"``: a tap whose source plane lies outside ``[0, nz)`` is
not formed, so it adds nothing (an ``inf`` there makes no NaN); any
``nz >= 1``.  ``z_boundary="periodic"``: the source plane index is taken
modulo ``nz``, which needs ``nz >= 2 rz + 1``.

Executors: the native one (default on the GPU) is ``csrc/stencil3d.hip``
through ``bridge.cpp:halo_stencil3d_nd`` / ``_dot_nd`` / ``_adjoint_nd``
with the launch sequences of the 2-D stencil.  The class only names these
three entries and lists the arguments they take before the exchange's
(``_native_args``); :class:`~.stencil.HaloStencil` makes the calls, so the
solvers of :mod:`.cg` and :mod:`.pcg` drive every stencil through the same
methods.  A block owns one 32 x 64
tile of one column and marches over ``z_chunk`` output planes with one
input plane resident in LDS and ``2 rz + 1`` output planes in registers.
The Python executor (the CPU path, or ``MPI4JAX_AMD_HALO_PY=1``) runs
``exchange`` and adds the taps in order by slicing on an ``Acc`` copy
viewed as ``(B, nz, ny, nx)``.  There is no 3-D Chebyshev kernel:
``make_chebyshev`` raises ``TypeError``.
"""

import torch

from .halo import HaloExchanger
from .stencil import MAX_RADIUS, TILE_Y, HaloStencil

MAX_TAPS = 32  # kStencil3dMaxTaps of csrc/kernels.h
MAX_RZ = 2     # kStencil3dMaxRz


def _parse_weights3d(weights):
    """``(rz, r, taps)`` of a ``(2rz+1, 2r+1, 2r+1)`` table; taps are
    ``(dz, dy, dx, coefficient)`` in row-major order with the zero weights
    dropped."""
    k = torch.as_tensor(weights)
    if k.is_complex():
        raise TypeError("stencil weights must be real")
    k = k.detach().to("cpu", torch.float64)
    if (k.dim() != 3 or k.shape[1] != k.shape[2] or k.shape[0] % 2 != 1
            or k.shape[1] % 2 != 1):
        raise ValueError(
            f"weights must be a (2rz+1, 2r+1, 2r+1) table, got shape "
            f"{tuple(k.shape)}")
    rz, r = (k.shape[0] - 1) // 2, (k.shape[1] - 1) // 2
    if rz > MAX_RZ:
        raise ValueError(f"z radius must be in 0..{MAX_RZ}, got {rz}")
    if not 1 <= r <= MAX_RADIUS:
        raise ValueError(
            f"stencil radius must be in 1..{MAX_RADIUS}, got {r}")
    taps = [(a - rz, b - r, c - r, k[a, b, c].item())
            for a in range(2 * rz + 1) for b in range(2 * r + 1)
            for c in range(2 * r + 1) if k[a, b, c].item() != 0.0]
    if not 1 <= len(taps) <= MAX_TAPS:
        raise ValueError(
            f"a 3-D stencil takes 1..{MAX_TAPS} non-zero weights, got "
            f"{len(taps)}")
    return rz, r, taps


class HaloStencil3D(HaloStencil):
    """See the module docstring.  Build with
    ``CartesianGrid.make_stencil3d``."""

    _APPLY = "halo_stencil3d_nd"
    _APPLY_DOT = "halo_stencil3d_dot_nd"
    _ADJOINT = "halo_stencil3d_adjoint_nd"

    def __init__(self, grid, shape, dtype, device, weights, nfields=1,
                 z_boundary="zero", _force_remote=False, _z_chunk=None):
        self._init_dtype(dtype)
        if z_boundary not in ("zero", "periodic"):
            raise ValueError(
                f"z_boundary must be 'zero' or 'periodic', got "
                f"{z_boundary!r}")
        self._rz, self._width, self._taps = _parse_weights3d(weights)
        shape = tuple(shape)
        if len(shape) < 3:
            raise ValueError(
                f"a 3-D stencil needs a shape (..., nz, ny, nx), got {shape}")
        self.nz = nz = int(shape[-3])
        self.z_boundary = z_boundary
        if z_boundary == "periodic" and nz < 2 * self._rz + 1:
            raise ValueError(
                f"periodic z needs nz >= 2*rz+1 = {2 * self._rz + 1}, got "
                f"nz = {nz}")
        self.exchanger = ex = HaloExchanger(
            grid, shape, dtype, device, width=self._width, nfields=nfields,
            _force_remote=_force_remote)
        self._tap_dz = [t[0] for t in self._taps]
        self._tap_dy = [t[1] for t in self._taps]
        self._tap_dx = [t[2] for t in self._taps]
        self._tap_coef = [t[3] for t in self._taps]
        self._zc = self._chunk(
            _z_chunk, "_z_chunk", nz,
            ex.nfields * (ex.levels // nz) * self._tiles(TILE_Y))

    @property
    def z_radius(self):
        """The table's radius ``rz`` along z."""
        return self._rz

    @property
    def taps(self):
        """``[(dz, dy, dx, coefficient), ...]`` in the order they are
        added."""
        return list(self._taps)

    @property
    def z_chunk(self):
        """Consecutive output planes one block of the native kernel marches
        over; it reads ``z_chunk + 2 rz`` input planes for them."""
        return self._zc

    def gershgorin_bounds(self):
        """``(centre - s, centre + s)``, ``s`` the sum of the magnitudes of
        the off-centre weights, as in
        :meth:`HaloStencil.gershgorin_bounds`.  The argument there holds
        for both z boundaries: with periodic z every row of ``A`` holds
        exactly these weights, and the zero boundary leaves a principal
        submatrix of that matrix."""
        c0 = sum(c for dz, dy, dx, c in self._taps
                 if (dz, dy, dx) == (0, 0, 0))
        s = sum(abs(c) for dz, dy, dx, c in self._taps
                if (dz, dy, dx) != (0, 0, 0))
        return float(c0 - s), float(c0 + s)

    def make_chebyshev(self, lmin, lmax):
        raise TypeError("make_chebyshev is 2-D only: the 3-D stencil has "
                        "no Chebyshev kernel yet")

    def make_line_solver(self, method="thomas", _lds_planes=None,
                         _pcr_columns=None):
        """A :class:`~.zline.ZLineSolver`: ``T^{-1}`` for the tridiagonal
        part ``T`` of this stencil along z (its ``(dz, 0, 0)`` weights).
        ``method="thomas"``: one thread marches over each column;
        ``"pcr"``: parallel cyclic reduction of a tile of columns in LDS,
        for tall columns on small planes (``ValueError`` for any other
        value, or for an ``nz`` whose columns do not fit in LDS).
        ``ValueError`` for a non-zero ``(+-2, 0, 0)`` weight or a ``T``
        whose factorisation meets a non-positive pivot; float32 and
        float64 only (``TypeError``)."""
        from .zline import ZLineSolver

        return ZLineSolver(self, _lds_planes=_lds_planes, method=method,
                           _pcr_columns=_pcr_columns)

    def make_cg(self, preconditioner=None, line_method="thomas",
                _lds_planes=None, _pcr_columns=None):
        """``preconditioner=None``: the :class:`~.cg.StencilCG` of
        ``HaloStencil.make_cg``.  ``"zline"``: a
        :class:`~.pcg.StencilPCG`, conjugate gradients preconditioned by
        the exact vertical line solve of :meth:`make_line_solver` with
        ``method=line_method``."""
        if preconditioner is None:
            return super().make_cg()
        if preconditioner != "zline":
            raise ValueError(
                f"preconditioner must be None or 'zline', got "
                f"{preconditioner!r}")
        from .pcg import StencilPCG

        return StencilPCG(self, _lds_planes=_lds_planes,
                          line_method=line_method, _pcr_columns=_pcr_columns)

    # ------------------------------------------------------------------
    def _native_args(self, ins, outs):
        ex = self.exchanger
        return (list(ins), list(outs), ex.levels, self.nz, ex.ny, ex.nx,
                self._width, self._tap_dz, self._tap_dy, self._tap_dx,
                self._tap_coef, self._zc, self.z_boundary == "periodic")

    def _z_terms(self, dz):
        """``(periodic, lo, hi)``: the planes ``k`` in ``[lo, hi)`` have a
        source plane ``k + dz`` under the zero boundary."""
        return (self.z_boundary == "periodic", max(0, -dz),
                min(self.nz, self.nz - dz))

    def _apply_py(self, fields, outs):
        ex = self.exchanger
        nz, ny, nx, w = self.nz, ex.ny, ex.nx, self._width
        exchanged = ex.exchange(*fields)
        if isinstance(exchanged, torch.Tensor):
            exchanged = (exchanged,)
        for e, o in zip(exchanged, outs):
            v = e.view(-1, nz, ny, nx).to(self.acc_dtype)
            acc = torch.zeros(v.shape[0], nz, ny - 2 * w, nx - 2 * w,
                              dtype=self.acc_dtype, device=e.device)
            for dz, dy, dx, c in self._taps:
                src = v[:, :, w + dy:ny - w + dy, w + dx:nx - w + dx]
                periodic, lo, hi = self._z_terms(dz)
                if periodic:
                    acc += c * torch.roll(src, -dz, 1)
                elif lo < hi:
                    acc[:, lo:hi] += c * src[:, lo + dz:hi + dz]
            o.view(-1, nz, ny, nx)[:, :, w:ny - w, w:nx - w].copy_(acc)

    def _adjoint_py(self, gouts, gins):
        ex = self.exchanger
        nz, ny, nx, w = self.nz, ex.ny, ex.nx, self._width
        for g, o in zip(gouts, gins):
            src = g.view(-1, nz, ny, nx)[:, :, w:ny - w, w:nx - w].to(
                self.acc_dtype)
            acc = torch.zeros(src.shape[0], nz, ny, nx,
                              dtype=self.acc_dtype, device=g.device)
            for dz, dy, dx, c in self._taps:
                dst = acc[:, :, w + dy:ny - w + dy, w + dx:nx - w + dx]
                periodic, lo, hi = self._z_terms(dz)
                if periodic:
                    dst += c * torch.roll(src, dz, 1)
                elif lo < hi:
                    dst[:, lo + dz:hi + dz] += c * src[:, lo:hi]
            o.view(-1, nz, ny, nx).copy_(acc)
        ex.adjoint_(*gins)
