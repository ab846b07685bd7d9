"""Per-column tridiagonal solves along z.

A :class:`ColumnTridiagonal` (built by
``CartesianGrid.make_tridiagonal_solver``) solves one tridiagonal system
per interior ``(j, i)`` of fields shaped ``(..., nz, ny, nx)``: row ``k`` of
column ``(j, i)`` is ``lower[k] x[k-1] + diag[k] x[k] + upper[k] x[k+1]``
with the bands three real ``(nz, ny, nx)`` tensors, local to the rank and
shared by every batch column and field.  ``lower[0]`` and ``upper[nz-1]``
are ignored, ``T`` need not be symmetric, and z is closed.  This is the
solve of implicit vertical mixing, ``(I - dt dz kappa dz) x = r`` with
``kappa(z, y, x)``; a column shallower than ``nz`` is expressed by identity
rows (``lower = upper = 0``, ``diag = 1``), which get no special treatment.
z is never decomposed, so nothing is communicated and no exchanger is
built; ``width`` only says how many halo cells per side in y and x are
left alone: they are never read in a right-hand side or a band and never
written in an output.

Factors.  ``set_bands`` runs the Thomas factorisation in float64 whatever
the field dtype, ``piv_0 = d_0``, ``piv_k = d_k - l_k cp_{k-1}``,
``inv_k = 1 / piv_k``, ``cp_k = u_k inv_k``, and rounds ``inv``, ``cp``
and a copy ``lo`` of the lower band once to the field dtype, into
``.factors`` (``(3, nz, ny, nx)``, halo cells zero).  A pivot of an
interior column that is not positive and finite raises ``ValueError``;
reading that status is the one host read of the set-up.  ``solve`` then
only multiplies:

* forward, ``k`` up: ``y_0 = r_0 inv_0``, ``y_k = (r_k - lo_k y_{k-1})
  inv_k``;
* back, ``k`` down: ``x_{nz-1} = y_{nz-1}``, ``x_k = y_k - cp_k x_{k+1}``.

``solve_bands`` is for bands that change every step: it factorises and
solves in one launch, leaves ``.factors`` alone, reads nothing back to the
host and checks no pivot, so a pivot that is not positive gives inf or
nan.  It computes the same factor values rounded the same way: on the same
bands it equals ``set_bands`` + ``solve`` bit for bit.

Executors.  The native one (``csrc/ztridiag.hip``) gives every interior
``(j, i)`` to one thread that marches over z and carries
``rhs_per_thread`` (1, 2 or 4) right-hand sides, so that the factor loads
are shared among them; a right-hand side is one (field, batch column)
pair.  ``y`` of the first ``lds_planes`` planes lives in LDS, of the
planes above in the output.  Results do not depend on either number.  The
Python executor (CPU, or ``MPI4JAX_AMD_HALO_PY=1``) runs the same
recurrences by slicing over planes.  The native kernels contract multiply
and add, so the two differ by rounding except where every operation is
exact.

float32 and float64 fields; bands may be float32 or float64 either way.
"""

import os

import torch

from .cg import CG_DTYPES
from .stencil import _span
from .zline import BLOCK, MAX_LDS, TILE_X, TILE_Y

MAX_FIELDS = 8              # kHaloMaxFields of csrc/kernels.h
RHS_PER_THREAD = (1, 2, 4)  # instantiations of csrc/ztridiag.hip


def _count(name, v, least):
    if isinstance(v, bool) or not isinstance(v, int) or v < least:
        raise ValueError(f"{name} must be an int >= {least}, got {v!r}")
    return v


class ColumnTridiagonal:
    """See the module docstring.  Build with
    ``CartesianGrid.make_tridiagonal_solver``."""

    def __init__(self, grid, shape, dtype, device, lower, diag, upper,
                 nfields=1, width=0, _rhs_per_thread=None, _lds_planes=None):
        shape = tuple(shape)
        if len(shape) < 3:
            raise ValueError(
                f"shape must be (..., nz, ny, nx), got {shape}")
        if dtype not in CG_DTYPES:
            raise TypeError(
                f"column solves support float32 and float64, got {dtype}")
        self._w = _count("width", width, 0)
        self._nf = _count("nfields", nfields, 1)
        if nfields > MAX_FIELDS:
            raise ValueError(
                f"nfields must be at most {MAX_FIELDS}, got {nfields}")
        self.grid, self.shape, self.dtype = grid, shape, dtype
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.nz, self.ny, self.nx = shape[-3:]
        if min(shape) < 1 or min(self.ny, self.nx) <= 2 * width:
            raise ValueError(
                f"shape {shape} has an empty interior at width {width}")
        self._batch = 1
        for n in shape[:-3]:
            self._batch *= n
        nrhs = self._nf * self._batch
        if _rhs_per_thread is None:
            # the largest that leaves no slot idle: sharing the factor
            # loads pays even where it pushes planes out of LDS
            # (docs/tuning.md has the measurements)
            _rhs_per_thread = max(r for r in RHS_PER_THREAD if r <= nrhs)
        elif (isinstance(_rhs_per_thread, bool)
              or _rhs_per_thread not in RHS_PER_THREAD):
            raise ValueError(
                f"_rhs_per_thread must be one of {RHS_PER_THREAD}, got "
                f"{_rhs_per_thread!r}")
        self._r = _rhs_per_thread
        if _lds_planes is not None and (
                isinstance(_lds_planes, bool)
                or not isinstance(_lds_planes, int)
                or not 0 <= _lds_planes <= self.nz):
            raise ValueError(
                f"_lds_planes must be an int in 0..{self.nz}, got "
                f"{_lds_planes!r}")
        most = self.nz if _lds_planes is None else _lds_planes
        # the fused path stashes cp_k next to the R values of y_k
        self._lds = min(most, self._fit(self._r))
        self._lds_fused = min(most, self._fit(self._r + 1))
        self._work = self._factors = None
        self.set_bands(lower, diag, upper)

    def _fit(self, slots):
        """Planes of ``slots`` values per thread that fit in LDS."""
        return MAX_LDS // (slots * BLOCK * self.dtype.itemsize)

    @property
    def factors(self):
        """The ``(3, nz, ny, nx)`` tensor of ``inv``, ``cp`` and ``lo`` in
        the field dtype; halo cells are zero."""
        return self._factors

    @property
    def lds_planes(self):
        """Planes whose ``y`` the native ``solve`` keeps in LDS; the planes
        above go through the output array."""
        return self._lds

    @property
    def rhs_per_thread(self):
        """Right-hand sides a thread of the native kernels carries through
        one march: 1, 2 or 4."""
        return self._r

    def set_bands(self, lower, diag, upper):
        """Factorise the bands into ``.factors``; raises ``ValueError`` for
        a pivot of an interior column that is not positive and finite."""
        bands = self._bands(lower, diag, upper)
        factors = torch.zeros((3,) + self.shape[-3:], dtype=self.dtype,
                              device=self.device)
        if self._native():
            from .._backend import rccl

            w = self._w
            tiles = (-(-(self.ny - 2 * w) // TILE_Y)
                     * -(-(self.nx - 2 * w) // TILE_X))
            status = torch.empty((tiles, 2), dtype=torch.float64,
                                 device=self.device)
            rccl.ext().ztridiag_factor_nd(*bands, factors, status,
                                          *self._geom())
            pivot, k = status[status[:, 0].argmin()].tolist()
        else:
            pivot, k = self._factor_py(bands, self._inner(factors), True)
        if not pivot > 0.0:
            raise ValueError(
                f"the bands are not positive definite along z: pivot "
                f"{int(k)} of a column (plane {int(k)}) is {pivot}")
        self._factors = factors

    def solve(self, *fields, out=None):
        """``T^{-1}`` on the interior columns of ``fields`` from the stored
        factors; the inputs are never mutated.  New tensors have a zero
        halo, and only the interior of ``out`` is written."""
        self._check(fields, "right-hand side")
        outs = self._outputs(fields, out)
        if self._native():
            from .._backend import rccl

            rccl.ext().ztridiag_solve_nd(
                list(fields), outs, self._factors, self._batch,
                *self._geom(), self._r, self._lds)
        else:
            inv, cp, lo = self._inner(self._factors)
            for r, x in zip(fields, outs):
                self._columns(x).copy_(
                    self._solve_py(self._columns(r), inv, cp, lo))
        return outs[0] if len(outs) == 1 else tuple(outs)

    def solve_bands(self, lower, diag, upper, *fields, out=None):
        """``solve`` for these bands instead of the stored factors, in one
        launch, without a host read and without a pivot check: a pivot that
        is not positive gives inf or nan.  ``.factors`` is not touched."""
        bands = self._bands(lower, diag, upper)
        self._check(fields, "right-hand side")
        outs = self._outputs(fields, out, bands)
        if self._native():
            from .._backend import rccl

            rccl.ext().ztridiag_solve_bands_nd(
                *bands, list(fields), outs, self._workspace(), self._batch,
                *self._geom(), self._r, self._lds_fused)
        else:
            w = self._w
            fac = torch.empty(
                (3, self.nz, self.ny - 2 * w, self.nx - 2 * w),
                dtype=self.dtype, device=self.device)
            self._factor_py(bands, fac, False)
            for r, x in zip(fields, outs):
                self._columns(x).copy_(self._solve_py(self._columns(r), *fac))
        return outs[0] if len(outs) == 1 else tuple(outs)

    # ------------------------------------------------------------------
    def _native(self):
        return (self.device.type == "cuda"
                and not os.environ.get("MPI4JAX_AMD_HALO_PY"))

    def _geom(self):
        return self.nz, self.ny, self.nx, self._w

    def _workspace(self):
        """``cp`` of the planes the fused kernel cannot stash, one copy per
        group of right-hand sides; allocated on first need."""
        spill = self.nz - self._lds_fused
        if spill > 0 and self._work is None:
            groups = -(-self._nf * self._batch // self._r)
            self._work = torch.empty(
                (groups, spill, self.ny, self.nx), dtype=self.dtype,
                device=self.device)
        return self._work if spill > 0 else torch.empty(
            0, dtype=self.dtype, device=self.device)

    def _bands(self, lower, diag, upper):
        """The three bands checked; contiguous and of one dtype for the
        native executor."""
        bands = (lower, diag, upper)
        for name, b in zip(("lower", "diag", "upper"), bands):
            if not isinstance(b, torch.Tensor):
                raise TypeError(
                    f"{name} must be a torch.Tensor, got {type(b)}")
            if b.dtype not in CG_DTYPES:
                raise TypeError(
                    f"{name} must be float32 or float64, got {b.dtype}")
            if tuple(b.shape) != self.shape[-3:]:
                raise ValueError(
                    f"{name} has shape {tuple(b.shape)}, expected "
                    f"{self.shape[-3:]}")
            if b.device != self.device:
                raise ValueError(
                    f"{name} lives on {b.device}, the solver on "
                    f"{self.device}")
        common = max((b.dtype for b in bands), key=lambda d: d.itemsize)
        return tuple(b.to(common).contiguous() for b in bands)

    def _check(self, fields, what):
        if len(fields) != self._nf:
            raise ValueError(
                f"the solver was built for {self._nf} field(s), got "
                f"{len(fields)} {what}(s)")
        for k, f in enumerate(fields):
            if not isinstance(f, torch.Tensor):
                raise TypeError(
                    f"{what} {k} must be a torch.Tensor, got {type(f)}")
            if (tuple(f.shape) != self.shape or f.dtype != self.dtype
                    or f.device != self.device):
                raise ValueError(
                    f"{what} {k} is {tuple(f.shape)} {f.dtype} on "
                    f"{f.device}, the solver was built for {self.shape} "
                    f"{self.dtype} on {self.device}")
            if not f.is_contiguous():
                raise ValueError(f"{what} {k} must be contiguous")

    def _outputs(self, ins, out, bands=()):
        if out is None:
            return [torch.zeros(self.shape, dtype=self.dtype,
                                device=self.device) for _ in ins]
        outs = [out] if isinstance(out, torch.Tensor) else list(out)
        self._check(outs, "output")
        read = [_span(t) for t in list(ins) + list(bands)]
        spans = read + [_span(t) for t in outs]
        for k in range(len(read), len(spans)):
            for j in range(k):
                if spans[k][0] < spans[j][1] and spans[j][0] < spans[k][1]:
                    raise ValueError(
                        f"out[{k - len(read)}] overlaps "
                        + (f"input {j}" if j < len(ins) else
                           "a band" if j < len(read)
                           else f"out[{j - len(read)}]"))
        return outs

    def _inner(self, t):
        """The interior of the last two axes."""
        w = self._w
        return t[..., w:self.ny - w, w:self.nx - w]

    def _columns(self, t):
        """The interior of ``t`` as ``(B, nz, ny - 2w, nx - 2w)``."""
        return self._inner(t.view(-1, self.nz, self.ny, self.nx))

    def _factor_py(self, bands, fac, check):
        """The float64 recurrence over planes on the interior; ``inv``,
        ``cp`` and ``lo`` rounded once into ``fac``.  With ``check``,
        returns the smallest pivot, a column counting up to its first one
        that is not positive and one that is not finite as -inf, and its
        plane."""
        lo, d, up = (self._inner(b).double() for b in bands)
        inf = float("inf")
        if check:
            low = torch.full_like(d[0], inf)
            low_k = torch.zeros_like(low)
            alive = torch.ones_like(low, dtype=torch.bool)
        cp = None
        for k in range(self.nz):
            pivot = d[k] if k == 0 else d[k] - lo[k] * cp
            inv = 1.0 / pivot
            cp = up[k] * inv
            fac[0, k], fac[1, k], fac[2, k] = inv, cp, lo[k]
            if check:
                m = torch.where(torch.isfinite(pivot), pivot,
                                torch.full_like(pivot, -inf))
                take = alive & (m < low)
                low = torch.where(take, m, low)
                low_k = torch.where(take, torch.full_like(low_k, k), low_k)
                alive = alive & (m > 0.0)
        if check:
            at = low.argmin()
            return torch.stack((low.flatten()[at],
                                low_k.flatten()[at])).tolist()
        return None

    def _solve_py(self, r, inv, cp, lo):
        y = torch.empty_like(r)
        y[:, 0] = r[:, 0] * inv[0]
        for k in range(1, self.nz):
            y[:, k] = (r[:, k] - lo[k] * y[:, k - 1]) * inv[k]
        for k in range(self.nz - 2, -1, -1):
            y[:, k] -= cp[k] * y[:, k + 1]
        return y
