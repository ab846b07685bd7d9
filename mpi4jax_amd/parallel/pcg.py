"""Vertical-line preconditioned conjugate gradients over a
:class:`~.stencil3d.HaloStencil3D`.

A :class:`StencilPCG` (built by ``HaloStencil3D.make_cg("zline")``) is
:class:`~.cg.StencilCG` with the preconditioner ``M = T``, the exact
vertical tridiagonal part of ``A`` (:mod:`.zline`).  It is for columns
whose z coupling is much stronger than the horizontal one, where plain
CG's iteration count grows with the anisotropy and this one's does not.
``M`` needs no communication and no extra reduction round, because z is
never decomposed.  Everything :class:`~.cg.StencilCG` says about ``A``,
boundary data, dtypes, scalars on the device, graph capture and
reproducibility holds here; ``T`` must be positive definite as well, which
the factorisation checks.

One iteration is three steps, each one native launch (plus one-block
finish launches after the reductions) when the fields live on the GPU:

1. ``q = A p`` and ``pq = p . q`` — the step of ``StencilCG``, unchanged;
2. ``alpha = rz / pq``; ``x += alpha p``; ``r -= alpha q``;
   ``z = M^{-1} r``; ``rr = r . r``; ``rz_old = rz``; ``rz = r . z`` on the
   stored ``r`` and ``z`` — ONE launch of ``csrc/zline.hip`` (or, with
   ``line_method="pcr"``, of ``csrc/zline_pcr.hip``): the line solve
   needs whole columns of the new ``r``, which the update produces plane
   by plane;
3. ``beta = rz / rz_old``; ``p = z + beta p`` — the direction kernel of
   ``StencilCG`` on ``z``.

With more ranks ``rz`` and ``rr`` pass through ``allreduce(SUM)`` after
step 2.  ``solve`` tests ``sqrt(rr)``, the residual's own 2-norm, exactly
as ``StencilCG.solve`` does.
"""

import torch

from .cg import StencilCG


class StencilPCG(StencilCG):
    """See the module docstring.  Build with
    ``HaloStencil3D.make_cg("zline")``."""

    def __init__(self, stencil, _lds_planes=None, line_method="thomas",
                 _pcr_columns=None):
        super().__init__(stencil)
        self.line_solver = stencil.make_line_solver(
            line_method, _lds_planes=_lds_planes, _pcr_columns=_pcr_columns)
        ex = stencil.exchanger
        # halo zero, never written
        self._z = [torch.zeros(ex.shape, dtype=ex.dtype, device=ex.device)
                   for _ in range(ex.nfields)]
        self._d = self._z
        self._rr = torch.zeros_like(self._rs)
        self._res2 = self._rr

    # ``_rs`` / ``_rs_old`` of the base class hold r . z here, so that its
    # alpha, beta and direction step apply unchanged.
    @property
    def rz(self):
        """The current global ``r . z`` (0-d float64 device tensor); it is
        also what :attr:`rs` returns."""
        return self._rs

    @property
    def rz_old(self):
        """``rz`` before the last update step."""
        return self._rs_old

    @property
    def rr(self):
        """The current global ``r . r`` of the recurrence (0-d float64
        device tensor), which ``solve`` tests."""
        return self._rr

    @property
    def preconditioned_residual(self):
        """``z = M^{-1} r``, as :attr:`residual`."""
        return self.stencil._ret(self._z)

    def start(self, b, x):
        """As ``StencilCG.start``, then ``z = M^{-1} r``, ``p = z``,
        ``rz = r . z`` and ``rr = r . r``."""
        super().start(b, x)
        st = self.stencil
        self._rr.copy_(self._rs)
        self.line_solver._solve_into(self._r, self._z)
        for fp, fz in zip(self._p, self._z):
            st._interior(fp).copy_(st._interior(fz))
        st._dot_into(self._r, self._z, self._rs)

    def update_step(self):
        """``alpha = rz / pq`` (0 when ``pq == 0``); ``x += alpha p``;
        ``r -= alpha q``; ``z = M^{-1} r``; ``rr = r . r``;
        ``rz_old = rz``; ``rz = r . z``."""
        self._started()
        self.line_solver._pcg_update(
            self._x, self._r, self._p, self._q, self._z, self._rs, self._pq,
            self._rs_old, self._rr)
        self.stencil._allreduce_(self._rs)
        self.stencil._allreduce_(self._rr)
