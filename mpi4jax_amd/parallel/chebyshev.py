"""Chebyshev iteration over a :class:`~.stencil.HaloStencil`.

A :class:`StencilChebyshev` (built by ``HaloStencil.make_chebyshev``)
solves ``A x = b`` for the interior cells of ``nfields`` decomposed fields
given bounds ``0 < lmin <= lambda(A) <= lmax`` on the eigenvalues of the
symmetric operator ``A`` (symmetric weights, every edge of the grid
periodic or closed).  Nothing checks the symmetry or the bounds; bounds
that leave an eigenvalue outside make the iteration diverge.
``HaloStencil.gershgorin_bounds`` gives rigorous ones for free, useful
whenever the stencil is diagonally dominant.

Unlike conjugate gradients the iteration needs no inner product.  With
``theta = (lmax + lmin) / 2``, ``delta = (lmax - lmin) / 2`` and
``sigma = theta / delta``, ``start`` sets ``r = b - A x`` and
``d = r / theta``, and iteration ``k = 0, 1, ...`` is

    ``q = A d;  x += d;  r -= q;  d' = c1 d + c2 r``

with ``rho_0 = 1 / sigma``, ``rho_{k+1} = 1 / (2 sigma - rho_k)``,
``c1 = rho_{k+1} rho_k`` and ``c2 = 2 rho_{k+1} / delta``.  The scalars
depend on ``k`` alone: the host computes them and passes them by value.
After ``k`` iterations ``||r_k|| <= ||r_0|| / T_k(sigma)`` in exact
arithmetic, ``T_k(s) = cosh(k acosh(s))`` (:meth:`iterations_for`).

On the GPU a whole iteration is ONE native launch — the stencil kernel
with its Chebyshev epilogue, ``csrc/bridge.cpp:halo_cheb_step_nd`` — that
reads ``d``, ``x``, ``r`` and writes ``x``, ``r``, ``d'``: six field-sized
streams, no reduction, and across ranks no collective besides the halo
exchange of ``d``.  ``iterate`` reads nothing from the device, allocates
nothing after a warm-up call and, on a one-rank grid, can be captured in a
``torch.cuda.graph``; a captured graph bakes in the coefficients of the
``k`` it was captured at, so replay it from the same ``k`` only (after a
fresh ``start``).

Boundary data is as for :class:`~.cg.StencilCG`: the solver never writes a
halo, the halos of ``r`` and ``d`` stay zero, and at a closed edge the halo
of ``x`` is Dirichlet data that enters through the first residual.

The Python executor (CPU, or ``MPI4JAX_AMD_HALO_PY=1``) does the same step
with the Python stencil and slicing, the same formulas in the same order;
on data where every operation is exact it agrees with the native executor
bitwise.  There is no reduction, so a decomposed run agrees with a
one-rank run bitwise.

float32 and float64 only.
"""

import math
from collections import namedtuple

import torch

from .stencil import _span

CHEBYSHEV_DTYPES = (torch.float32, torch.float64)

ChebyshevInfo = namedtuple("ChebyshevInfo",
                           "iterations converged residual_norm rhs_norm")
ChebyshevInfo.__doc__ = """Result of :meth:`StencilChebyshev.solve`:
``iterations`` run, ``converged``, and the 2-norms of the recurrence
residual and of ``b`` as floats.  With ``check_every=0`` no inner product
is computed: ``converged`` and both norms are ``None``."""


class StencilChebyshev:
    """See the module docstring.  Build with
    ``HaloStencil.make_chebyshev``."""

    def __init__(self, stencil, lmin, lmax):
        if stencil.dtype not in CHEBYSHEV_DTYPES:
            raise TypeError(
                f"Chebyshev iteration supports float32 and float64, the "
                f"stencil was built for {stencil.dtype}")
        for name, v in (("lmin", lmin), ("lmax", lmax)):
            if isinstance(v, bool) or not isinstance(v, (int, float)):
                raise TypeError(f"{name} must be a real number, got {v!r}")
        lmin, lmax = float(lmin), float(lmax)
        if not 0.0 < lmin < lmax < math.inf:
            raise ValueError(
                f"eigenvalue bounds must satisfy 0 < lmin < lmax < inf, "
                f"got ({lmin}, {lmax})")
        self.stencil = stencil
        self.lmin, self.lmax = lmin, lmax
        self.theta = (lmax + lmin) / 2
        self.delta = (lmax - lmin) / 2
        self.sigma = self.theta / self.delta
        ex = stencil.exchanger

        def fields():
            return [torch.zeros(ex.shape, dtype=ex.dtype, device=ex.device)
                    for _ in range(ex.nfields)]

        # halos zero, never written
        self._r = fields()
        self._d = [fields(), fields()]  # current direction: _d[_cur]
        self._cur = 0
        self._q = None  # Python executor only, see _step_py
        self._x = None
        self._k = 0
        self._rho = [1.0 / self.sigma]  # rho_0, rho_1, ... as needed

    @property
    def residual(self):
        """The recurrence residual ``r``: one tensor for one field, else a
        tuple; halos are zero."""
        return self.stencil._ret(self._r)

    @property
    def direction(self):
        """The current direction ``d``, as :attr:`residual`.  The two
        buffers alternate: after a step this is another tensor."""
        return self.stencil._ret(self._d[self._cur])

    @property
    def iteration(self):
        """``k``: the steps taken since the last :meth:`start`."""
        return self._k

    # ------------------------------------------------------------------
    def coefficients(self, k):
        """``(c1, c2)`` of iteration ``k`` (module docstring), as Python
        floats."""
        if isinstance(k, bool) or not isinstance(k, int) or k < 0:
            raise ValueError(f"k must be a non-negative int, got {k!r}")
        rho = self._rho
        while len(rho) < k + 2:
            rho.append(1.0 / (2.0 * self.sigma - rho[-1]))
        return rho[k + 1] * rho[k], 2.0 * rho[k + 1] / self.delta

    def iterations_for(self, rtol):
        """The smallest ``k`` with ``1 / T_k(sigma) <= rtol``: after that
        many iterations ``||r_k|| <= rtol * ||r_0||`` in exact
        arithmetic."""
        rtol = float(rtol)
        if not 0.0 < rtol:
            raise ValueError(f"rtol must be positive, got {rtol}")
        if rtol >= 1.0:
            return 0
        a = math.acosh(self.sigma)
        k = max(0, math.ceil(math.acosh(1.0 / rtol) / a) - 2)
        while 1.0 / math.cosh(k * a) > rtol:
            k += 1
        return k

    def start(self, b, x):
        """Begin a solve of ``A x = b`` from the current ``x``: ``r = b -
        A x`` on the interior, ``d = r / theta``, ``k = 0``.  ``b`` and
        ``x`` are each one tensor or a sequence of ``nfields`` tensors;
        the halo of ``b`` is ignored.  Later iterations update the
        interior of ``x`` in place; its halo is read where an edge is
        closed (Dirichlet data) and never written.  May allocate.  A
        collective."""
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
        self._cur = 0
        d, q = self._d[0], self._d[1]  # the other d buffer holds A x
        if st._native():
            st._call_native("halo_stencil_nd", x, q)
        else:
            st._apply_py(x, q)
        for fb, fr, fd, fq in zip(b, self._r, d, q):
            ri = st._interior(fr)
            torch.sub(st._interior(fb), st._interior(fq), out=ri)
            torch.div(ri, self.theta, out=st._interior(fd))
        self._x = list(x)
        self._k = 0

    def step(self, c1, c2):
        """One iteration with explicit coefficients: ``q = A d``,
        ``x += d``, ``r -= q``, ``d' = c1 d + c2 r``; ``d'`` goes to the
        other direction buffer, which becomes :attr:`direction`.  One
        native launch on the GPU.  A collective (the halo exchange of
        ``d``)."""
        self._started()
        c1, c2 = float(c1), float(c2)
        if not (math.isfinite(c1) and math.isfinite(c2)):
            raise ValueError(
                f"c1 and c2 must be finite, got {c1} and {c2}")
        d_in, d_out = self._d[self._cur], self._d[1 - self._cur]
        if self.stencil._native():
            self._step_native(d_in, d_out, c1, c2)
        else:
            self._step_py(d_in, d_out, c1, c2)
        self._cur = 1 - self._cur
        self._k += 1

    def iterate(self, n=1):
        """Run the next ``n`` iterations on the system of the last
        :meth:`start`: ``step(*coefficients(k))`` for ``k = iteration,
        ...``.  No host read; no allocation after a warm-up call."""
        if isinstance(n, bool) or not isinstance(n, int) or n < 0:
            raise ValueError(f"n must be a non-negative int, got {n!r}")
        self._started()
        for _ in range(n):
            self.step(*self.coefficients(self._k))

    def solve(self, b, x0=None, *, rtol=1e-6, atol=0.0, maxiter=None,
              check_every=8):
        """Solve ``A x = b``; returns ``(x, ChebyshevInfo)`` with ``x``
        new tensors (one for one field, else a tuple): a copy of ``x0``,
        halo included, or zeros, with the interior solved for.
        ``maxiter=None`` means ``iterations_for(rtol)`` (at least 1).
        Stops when ``sqrt(r . r) <= max(rtol * ||b||, atol)``, tested
        through ``HaloStencil.dot`` (one host read) after every
        ``check_every`` iterations and at ``maxiter``.  ``check_every=0``
        runs exactly ``maxiter`` iterations and computes no inner product
        and no allreduce at all, so the norms of the result are ``None``.
        A non-finite residual at a test raises ``FloatingPointError``.  A
        collective: every rank calls it with the same arguments."""
        if maxiter is None:
            maxiter = max(1, self.iterations_for(rtol))
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
        self.start(b, x)
        if check_every == 0:
            self.iterate(maxiter)
            return st._ret(x), ChebyshevInfo(maxiter, None, None, None)
        bnorm = math.sqrt(self._finite(st._dot_into(b, b, st._scalar()),
                                       "b . b"))
        tol = max(rtol * bnorm, atol)
        rr = st._scalar()
        done, converged = 0, False
        while done < maxiter and not converged:
            n = min(check_every, maxiter - done)
            self.iterate(n)
            done += n
            rnorm = math.sqrt(self._finite(
                st._dot_into(self._r, self._r, rr), "r . r"))
            converged = rnorm <= tol
        return st._ret(x), ChebyshevInfo(done, converged, rnorm, bnorm)

    # ------------------------------------------------------------------
    def _started(self):
        if self._x is None:
            raise RuntimeError(
                "StencilChebyshev: call start (or solve) first")

    @staticmethod
    def _finite(scalar, what):
        v = scalar.item()  # the host read
        if not math.isfinite(v) or v < 0.0:
            raise FloatingPointError(
                f"Chebyshev iteration: {what} = {v}; do the bounds hold "
                f"every eigenvalue of the operator?")
        return v

    def _step_native(self, d_in, d_out, c1, c2):
        from .._backend import rccl

        st = self.stencil
        ex = st.exchanger
        comm_id = rccl._handle(ex.comm) if ex._has_remote else -1
        rccl.ext().halo_cheb_step_nd(
            d_in, d_out, self._x, self._r, ex.levels, ex.ny, ex.nx,
            st.width, st._tap_dy, st._tap_dx, st._tap_coef, ex._send_to,
            ex._recv_from, ex._local_mask, ex._sbuf, ex._rbuf, comm_id,
            c1, c2)

    def _step_py(self, d_in, d_out, c1, c2):
        st = self.stencil
        if self._q is None:
            self._q = [torch.zeros_like(t) for t in self._r]
        st._apply_py(d_in, self._q)
        for fx, fr, fd, fn, fq in zip(self._x, self._r, d_in, d_out,
                                      self._q):
            di, ri = st._interior(fd), st._interior(fr)
            st._interior(fx).add_(di)
            ri.sub_(st._interior(fq))
            torch.add(c1 * di, c2 * ri, out=st._interior(fn))
