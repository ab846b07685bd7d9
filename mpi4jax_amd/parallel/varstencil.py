"""Variable-coefficient halo stencil: ``HaloStencil`` with one coefficient
plane per tap instead of one constant.

A :class:`VariableHaloStencil` (built by
``CartesianGrid.make_variable_stencil``) takes ``1 <= T <= 13`` distinct
offsets ``(dy, dx)`` and a real tensor ``coefficients`` of shape
``(T, ny, nx)``: plane ``t`` holds ``K_t``, local to the rank, on the same
``(ny, nx)`` grid as the fields and shared by every level and every field.
The radius ``r = max(|dy|, |dx|)``, ``1 <= r <= 4``, is the halo width.
With ``E`` and ``P_int`` exactly as in :mod:`.stencil`:

* ``apply`` is ``A = P_int . S_K . E`` with
  ``out[l, j, i] = sum_t K_t[j, i] * v[l, j + dy_t, i + dx_t]``, the sum
  formed in the accumulate type ``Acc`` from 0 in the order of ``offsets``
  and rounded once at a 16-bit store;
* ``adjoint`` is ``A^T = E^T . S_K^T . P_int``: ``S_K^T`` writes every cell
  ``p`` of the full array with the sum, in the same order and from 0, of
  ``K_t[p - o_t] * gout[p - o_t]`` over the taps whose source cell
  ``p - o_t`` is interior;
* ``apply_dot``, ``dot``, ``apply_ad`` and ``make_cg`` are inherited from
  :class:`~.stencil.HaloStencil`.  CG needs a symmetric operator, which is
  the caller's business: ``K_t[c] == K_{-t}[c + o_t]`` for every cell
  ``c``, across rank edges too.

Only interior cells of a coefficient plane are ever read, so the halo of
``coefficients`` may hold anything.  Unlike the constant stencil nothing
drops zeros per cell: ``0 * inf`` is NaN here.

The stencil keeps its own contiguous copy of the coefficients in ``Acc``
on the fields' device; :meth:`VariableHaloStencil.set_coefficients`
overwrites it in place.

Executors: the native one (default on the GPU) is ``csrc/varstencil.hip``
through ``bridge.cpp:halo_varstencil_nd`` / ``_dot_nd`` / ``_adjoint_nd``,
with the launch sequences of the constant stencil.  The class only names
these three entries and lists the arguments they take before the
exchange's (``_native_args``); :class:`~.stencil.HaloStencil` makes the
calls, so the solvers of :mod:`.cg` drive every stencil through the same
methods.  A block keeps the
coefficients of its tile in registers while it marches over
``levels_per_block`` consecutive levels, so coefficient traffic does not
grow with the number of levels.  The Python executor (the CPU path, or
``MPI4JAX_AMD_HALO_PY=1``) runs ``exchange`` and adds the taps in order by
slicing on an ``Acc`` copy.  ``make_chebyshev`` and ``gershgorin_bounds``
are constant-coefficient only and raise ``TypeError``.
"""

import torch

from .stencil import MAX_RADIUS, TILE_Y, HaloStencil
from .halo import HaloExchanger

MAX_TAPS = 13  # kVarStencilMaxTaps of csrc/kernels.h
# rows of a tile by accumulate type: 4 * kVarStencilRowsF32 / F64
_TILE_Y = {torch.float32: 32, torch.float64: 16}


def _parse_offsets(offsets):
    try:
        given = [tuple(o) for o in offsets]
        offs = [(int(dy), int(dx)) for dy, dx in given]
    except (TypeError, ValueError):
        raise TypeError("offsets must be a sequence of (dy, dx) pairs of "
                        "ints") from None
    if offs != given:
        raise TypeError(f"offsets must be ints, got {given}")
    if not 1 <= len(offs) <= MAX_TAPS:
        raise ValueError(
            f"a variable stencil takes 1..{MAX_TAPS} taps, got {len(offs)}")
    if len(set(offs)) != len(offs):
        raise ValueError(f"duplicate offsets in {offs}")
    r = max(max(abs(dy), abs(dx)) for dy, dx in offs)
    if not 1 <= r <= MAX_RADIUS:
        raise ValueError(
            f"stencil radius must be in 1..{MAX_RADIUS}, got {r}")
    return r, offs


class VariableHaloStencil(HaloStencil):
    """See the module docstring.  Build with
    ``CartesianGrid.make_variable_stencil``."""

    _APPLY = "halo_varstencil_nd"
    _APPLY_DOT = "halo_varstencil_dot_nd"
    _ADJOINT = "halo_varstencil_adjoint_nd"

    def __init__(self, grid, shape, dtype, device, offsets, coefficients,
                 nfields=1, _force_remote=False, _levels_per_block=None):
        self._init_dtype(dtype)
        self._width, self._offsets = _parse_offsets(offsets)
        self._tap_dy = [o[0] for o in self._offsets]
        self._tap_dx = [o[1] for o in self._offsets]
        shape = tuple(shape)
        self._coef_shape = (len(self._offsets),) + shape[-2:]
        self._check_coefficients(coefficients)
        self.exchanger = ex = HaloExchanger(
            grid, shape, dtype, device, width=self._width, nfields=nfields,
            _force_remote=_force_remote)
        self._coef = torch.empty(self._coef_shape, dtype=self.acc_dtype,
                                 device=ex.device)
        self._coef.copy_(coefficients.detach())
        self._lpb = self._chunk(
            _levels_per_block, "_levels_per_block", ex.levels,
            ex.nfields * self._tiles(_TILE_Y[self.acc_dtype]))

    def _check_coefficients(self, c):
        if not isinstance(c, torch.Tensor):
            raise TypeError("coefficients must be a tensor")
        if c.is_complex():
            raise TypeError(f"coefficients must be real, got {c.dtype}")
        if tuple(c.shape) != self._coef_shape:
            raise ValueError(
                f"coefficients must have shape {self._coef_shape} (one "
                f"(ny, nx) plane per tap), got {tuple(c.shape)}")

    def set_coefficients(self, coefficients):
        """Overwrite the stencil's copy of the coefficients in place with a
        real tensor of the same ``(T, ny, nx)`` shape (``TypeError`` /
        ``ValueError`` otherwise).  Nothing is reallocated or rebuilt."""
        self._check_coefficients(coefficients)
        self._coef.copy_(coefficients.detach())

    @property
    def offsets(self):
        """``[(dy, dx), ...]`` in the order the taps are added."""
        return list(self._offsets)

    @property
    def coefficients(self):
        """The stencil's own ``(T, ny, nx)`` copy in ``Acc`` (not a copy of
        it: writes show in later calls)."""
        return self._coef

    @property
    def levels_per_block(self):
        """Consecutive levels one block of the native kernel marches
        over."""
        return self._lpb

    @property
    def taps(self):
        raise TypeError("a variable stencil has offsets and coefficients, "
                        "not constant taps")

    def gershgorin_bounds(self):
        raise TypeError("gershgorin_bounds is constant-coefficient only: "
                        "use HaloStencil, or bound the operator yourself")

    def make_chebyshev(self, lmin, lmax):
        raise TypeError("make_chebyshev is constant-coefficient only: the "
                        "variable stencil has no Chebyshev kernel yet")

    # ------------------------------------------------------------------
    def _partials_buf(self):
        """One float64 slot per block of the largest native grid: the
        Krylov kernels' 32 x 64 tiles of every plane, or this kernel's
        tiles with one level per block."""
        if self._partials is None:
            ex = self.exchanger
            tiles = max(self._tiles(TILE_Y),
                        self._tiles(_TILE_Y[self.acc_dtype]))
            self._partials = torch.empty(
                ex.nfields * ex.levels * tiles, dtype=torch.float64,
                device=ex.device)
        return self._partials

    def _native_args(self, ins, outs):
        ex = self.exchanger
        return (list(ins), list(outs), ex.levels, ex.ny, ex.nx, self._width,
                self._tap_dy, self._tap_dx, self._coef, self._lpb)

    def _apply_py(self, fields, outs):
        ex = self.exchanger
        L, ny, nx, w = ex.levels, ex.ny, ex.nx, self._width
        exchanged = ex.exchange(*fields)
        if isinstance(exchanged, torch.Tensor):
            exchanged = (exchanged,)
        ki = self._coef[:, w:ny - w, w:nx - w]
        for e, o in zip(exchanged, outs):
            v = e.view(L, ny, nx).to(self.acc_dtype)
            acc = torch.zeros(L, ny - 2 * w, nx - 2 * w,
                              dtype=self.acc_dtype, device=e.device)
            for t, (dy, dx) in enumerate(self._offsets):
                acc += ki[t] * v[:, w + dy:ny - w + dy, w + dx:nx - w + dx]
            o.view(L, ny, nx)[:, w:ny - w, w:nx - w].copy_(acc)

    def _adjoint_py(self, gouts, gins):
        ex = self.exchanger
        L, ny, nx, w = ex.levels, ex.ny, ex.nx, self._width
        ki = self._coef[:, w:ny - w, w:nx - w]
        for g, o in zip(gouts, gins):
            src = g.view(L, ny, nx)[:, w:ny - w, w:nx - w].to(self.acc_dtype)
            acc = torch.zeros(L, ny, nx, dtype=self.acc_dtype,
                              device=g.device)
            for t, (dy, dx) in enumerate(self._offsets):
                acc[:, w + dy:ny - w + dy, w + dx:nx - w + dx] += ki[t] * src
            o.view(L, ny, nx).copy_(acc)
        ex.adjoint_(*gins)
