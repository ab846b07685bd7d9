"""Conjugate gradients over a :class:`~.stencil.HaloStencil`.

A :class:`StencilCG` (built by ``HaloStencil.make_cg``) solves ``A x = b``
for the interior cells of ``nfields`` decomposed fields, all fields
together as ONE vector with one ``alpha`` and one ``beta`` per iteration.
``A`` must be symmetric positive definite on interior vectors: symmetric
weights, every edge of the grid periodic or closed.  Nothing checks that.

Boundary data.  ``A`` reads the halo of ``x`` wherever an edge is closed,
and the solver never writes a halo.  The halo of the search direction
``p`` stays zero, so at a closed edge the halo of ``x`` is Dirichlet data:
the iteration solves for the interior with those values held fixed (they
enter through the first residual ``b - A x``).  At periodic or decomposed
edges halo cells are read from the neighbour's interior as always and
their stored values do not matter.

One iteration is three steps, each a native launch (plus a one-block
finish launch after the two that reduce) when the fields live on the GPU:

1. ``q = A p`` and ``pq = p . q`` — ``HaloStencil.apply_dot``'s kernel;
2. ``alpha = rs / pq``; ``x += alpha p``; ``r -= alpha q``;
   ``rs_old = rs``; ``rs = r . r`` on the stored ``r``;
3. ``beta = rs / rs_old``; ``p = r + beta p``.

``rs``, ``rs_old`` and ``pq`` are float64 scalars that stay on the device:
``iterate`` reads nothing back, allocates nothing after a warm-up call and,
on a one-rank grid, can be captured in a ``torch.cuda.graph``.  With more
ranks ``pq`` and ``rs`` pass through ``allreduce(SUM)``.  ``alpha`` and
``beta`` are formed in float64 and rounded once to the field dtype; a zero
denominator gives 0, so iterating past exact convergence changes nothing
and makes no NaN.  Inner products are those of ``HaloStencil.dot``:
float64, one fixed order, no atomics — two solves of the same system agree
bitwise.

The Python executor (CPU, or ``MPI4JAX_AMD_HALO_PY=1``) runs the same
three steps with torch slicing; on data whose products are exact it agrees
with the native executor bitwise.

float32 and float64 only: CG in 16-bit storage is not offered.
"""

import math
from collections import namedtuple

import torch

from .stencil import _span

CG_DTYPES = (torch.float32, torch.float64)

CGInfo = namedtuple("CGInfo",
                    "iterations converged residual_norm rhs_norm")
CGInfo.__doc__ = """Result of :meth:`StencilCG.solve`: ``iterations`` run,
``converged`` (``None`` with ``check_every=0``), and the 2-norms of the
recurrence residual and of ``b`` — floats, or 0-d device tensors with
``check_every=0``, which reads nothing back."""


class StencilCG:
    """See the module docstring.  Build with ``HaloStencil.make_cg``."""

    def __init__(self, stencil):
        if stencil.dtype not in CG_DTYPES:
            raise TypeError(
                f"conjugate gradients support float32 and float64, the "
                f"stencil was built for {stencil.dtype}")
        self.stencil = stencil
        ex = stencil.exchanger

        def fields():
            return [torch.zeros(ex.shape, dtype=ex.dtype, device=ex.device)
                    for _ in range(ex.nfields)]

        # halos zero, never written
        self._r, self._p, self._q = fields(), fields(), fields()
        self._x = None
        self._rs = torch.zeros((), dtype=torch.float64, device=ex.device)
        self._rs_old = torch.zeros_like(self._rs)
        self._pq = torch.zeros_like(self._rs)

    @property
    def rs(self):
        """The current global ``r . r`` of the recurrence: a 0-d float64
        device tensor, updated in place by ``iterate``."""
        return self._rs

    @property
    def rs_old(self):
        """``rs`` before the last update step (0-d float64 device tensor)."""
        return self._rs_old

    @property
    def pq(self):
        """The global ``p . A p`` of the last apply step (0-d float64
        device tensor)."""
        return self._pq

    @property
    def direction(self):
        """The search direction ``p``, as :attr:`residual`."""
        return self.stencil._ret(self._p)

    @property
    def residual(self):
        """The recurrence residual ``r``: one tensor for one field, else a
        tuple; halos are zero."""
        return self.stencil._ret(self._r)

    # ------------------------------------------------------------------
    def start(self, b, x):
        """Begin a solve of ``A x = b`` from the current ``x``: ``r = b -
        A x`` on the interior, ``p = r``, ``rs = r . r``.  ``b`` and ``x``
        are each one tensor or a sequence of ``nfields`` tensors; the halo
        of ``b`` is ignored.  Later iterations update the interior of
        ``x`` in place; its halo is read where an edge is closed
        (Dirichlet data, see the module docstring) and never written.
        May allocate.  A collective."""
        st = self.stencil
        b, x = st._field_list(b), st._field_list(x)
        spans = [_span(t) for t in x + b]
        for k in range(len(x)):
            for j in range(len(spans)):
                if j != k and (spans[k][0] < spans[j][1]
                               and spans[j][0] < spans[k][1]):
                    raise ValueError(
                        f"x[{k}] overlaps "
                        + (f"x[{j}]" if j < len(x) else f"b[{j - len(x)}]"))
        if st._native():  # q = A x
            st._call_native("halo_stencil_nd", x, self._q)
        else:
            st._apply_py(x, self._q)
        for fb, fr, fp, fq in zip(b, self._r, self._p, self._q):
            ri = st._interior(fr)
            torch.sub(st._interior(fb), st._interior(fq), out=ri)
            st._interior(fp).copy_(ri)
        self._x = list(x)
        self._rs_old.zero_()
        st._dot_into(self._r, self._r, self._rs)

    def iterate(self, n=1):
        """Run ``n`` iterations on the system of the last :meth:`start`.
        No host read; no allocation after a warm-up call."""
        if isinstance(n, bool) or not isinstance(n, int) or n < 0:
            raise ValueError(f"n must be a non-negative int, got {n!r}")
        self._started()
        for _ in range(n):
            self.apply_step()
            self.update_step()
            self.direction_step()

    # The three steps of one iteration, in the order iterate runs them.
    # Public so that a variant of the iteration can be composed from them
    # and so that each can be tested alone; every one is a collective.
    def apply_step(self):
        """``q = A p`` and ``pq = p . q``."""
        self._started()
        self.stencil._apply_dot_into(self._p, self._q, self._pq)

    def update_step(self):
        """``alpha = rs / pq`` (0 when ``pq == 0``); ``x += alpha p``;
        ``r -= alpha q``; ``rs_old = rs``; ``rs = r . r``."""
        self._started()
        if self.stencil._native():
            self._update_native()
        else:
            self._update_py()
        self.stencil._allreduce_(self._rs)

    def direction_step(self):
        """``beta = rs / rs_old`` (0 when ``rs_old == 0``);
        ``p = r + beta p``."""
        self._started()
        if self.stencil._native():
            self._direction_native()
        else:
            self._direction_py()

    def solve(self, b, x0=None, *, rtol=1e-6, atol=0.0, maxiter,
              check_every=8):
        """Solve ``A x = b``; returns ``(x, CGInfo)`` with ``x`` new
        tensors (one for one field, else a tuple): a copy of ``x0``, halo
        included, or zeros, with the interior solved for.  Stops when
        ``sqrt(rs) <= max(rtol * ||b||, atol)``, which is tested by one
        host read after every ``check_every`` iterations and at
        ``maxiter``.  ``check_every=0`` runs exactly ``maxiter``
        iterations with no host read.  A non-finite ``rs`` at a test
        raises ``FloatingPointError``.  A collective: every rank calls it
        with the same arguments."""
        for name, v in (("maxiter", maxiter), ("check_every", check_every)):
            if isinstance(v, bool) or not isinstance(v, int):
                raise TypeError(f"{name} must be an int, got {v!r}")
        if maxiter < 1:
            raise ValueError(f"maxiter must be >= 1, got {maxiter}")
        if check_every < 0:
            raise ValueError(f"check_every must be >= 0, got {check_every}")
        st = self.stencil
        b = st._field_list(b)
        if x0 is None:
            x = [torch.zeros_like(f) for f in b]
        else:
            x = [f.clone() for f in st._field_list(x0)]
        bb = st._dot_into(b, b, st._scalar())
        self.start(b, x)
        if check_every == 0:
            self.iterate(maxiter)
            return st._ret(x), CGInfo(maxiter, None, self._rs.sqrt(),
                                      bb.sqrt())
        bnorm = math.sqrt(self._finite(bb, "b . b"))
        tol = max(rtol * bnorm, atol)
        done, converged = 0, False
        while done < maxiter and not converged:
            n = min(check_every, maxiter - done)
            self.iterate(n)
            done += n
            rnorm = math.sqrt(self._finite(self._rs, "r . r"))
            converged = rnorm <= tol
        return st._ret(x), CGInfo(done, converged, rnorm, bnorm)

    # ------------------------------------------------------------------
    def _started(self):
        if self._x is None:
            raise RuntimeError("StencilCG: call start (or solve) first")

    @staticmethod
    def _finite(scalar, what):
        v = scalar.item()  # the host read
        if not math.isfinite(v) or v < 0.0:
            raise FloatingPointError(
                f"conjugate gradients: {what} = {v}; is the operator "
                f"symmetric positive definite?")
        return v

    def _geom(self):
        ex = self.stencil.exchanger
        return ex.levels, ex.ny, ex.nx, self.stencil.width

    def _update_native(self):
        from .._backend import rccl

        rccl.ext().halo_cg_update_nd(
            self._x, self._r, self._p, self._q, *self._geom(), self._rs,
            self._pq, self._rs_old, self.stencil._partials_buf())

    def _direction_native(self):
        from .._backend import rccl

        rccl.ext().halo_cg_direction_nd(
            self._p, self._r, *self._geom(), self._rs, self._rs_old)

    def _ratio(self, num, den):
        """``num / den`` in float64, 0 where ``den == 0``, rounded once to
        the accumulate type; a 0-d device tensor, nothing read back."""
        q = torch.where(den == 0, torch.zeros_like(num), num / den)
        return q.to(self.stencil.acc_dtype)

    def _update_py(self):
        st = self.stencil
        alpha = self._ratio(self._rs, self._pq)
        total = None
        for fx, fr, fp, fq in zip(self._x, self._r, self._p, self._q):
            st._interior(fx).add_(alpha * st._interior(fp))
            ri = st._interior(fr)
            ri.sub_(alpha * st._interior(fq))
            s = (ri.double() * ri.double()).sum()
            total = s if total is None else total + s
        self._rs_old.copy_(self._rs)
        self._rs.copy_(total)

    def _direction_py(self):
        st = self.stencil
        beta = self._ratio(self._rs, self._rs_old)
        for fr, fp in zip(self._r, self._p):
            pi = st._interior(fp)
            torch.add(st._interior(fr), beta * pi, out=pi)
