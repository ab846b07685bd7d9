"""Fused halo stencil: a constant-coefficient stencil applied through the
halo exchange as one linear operator, with a native adjoint.

A :class:`HaloStencil` (built by ``CartesianGrid.make_stencil``) owns a
:class:`~.halo.HaloExchanger` of halo width ``r`` and a ``(2r+1, 2r+1)``
table of real weights, ``1 <= r <= 4``.  Entry ``[a][b]`` multiplies the
cell at offset ``(a - r, b - r)`` in ``(y, x)``.  The operator is

    ``A = P_int . S . E``

* ``E`` is the exchanger's ``exchange`` with exactly its semantics — also
  where they are asymmetric: with y periodic and x closed the halo corner
  blocks keep their own values, because row strips cover the interior
  columns only;
* ``S`` computes, for every interior cell ``(j, i)``, ``w <= j < ny - w``
  and ``w <= i < nx - w``, ``sum_t K_t * v[j + dy_t, i + dx_t]``.  The sum
  is formed in the accumulate type ``Acc`` (float32 for float16, bfloat16
  and float32 fields, float64 for float64 fields), starts from 0 and takes
  the taps in row-major ``(a, b)`` order; float16 / bfloat16 are rounded
  once, at the store;
* ``P_int``: only interior cells of the output are written.

Zero weights are dropped when the stencil is built, so no executor ever
multiplies by one: an ``inf`` under a zero weight does not make a NaN.

``adjoint`` is ``A^T = E^T . S^T . P_int``.  ``S^T`` writes every cell
``p`` of the full array, halo included: ``gin[p]`` is the sum over the
taps, in the same order and from 0, of ``K_t * gout[p - (dy_t, dx_t)]``
counting only terms whose source cell is interior.  ``E^T`` is then
``HaloExchanger.adjoint_`` in place on that result.

Executors:

* the **native** executor (default on the GPU) is one call into
  ``csrc/bridge.cpp:halo_stencil_nd`` / ``halo_stencil_adjoint_nd``.  With
  no remote peer ``apply`` is ONE kernel launch that reads every halo cell
  from where ``exchange`` would have copied it; nothing is staged and no
  communicator is created.  With a remote peer it is the exchanger's pack
  launch, the exchanger's RCCL group and one stencil launch that reads
  halo cells from the receive staging slots.  The input is never written;
* the **Python** executor (any device; the CPU path; forced on the GPU by
  ``MPI4JAX_AMD_HALO_PY=1``) runs ``exchange`` and adds the taps in order
  by slicing on an ``Acc`` copy.

On integer-valued data the executors agree bitwise.  On other data the GPU
kernel contracts multiply and add into a fused multiply-add, so CPU and
GPU results differ by rounding.

``apply`` and ``adjoint`` are not differentiable.  ``apply_ad`` is: its
backward pass is ``adjoint``, a collective with the caveats of
``HaloExchanger.exchange_ad``.
"""

import os

import torch
from torch.autograd.function import once_differentiable

from .halo import AD_DTYPES, HaloExchanger

MAX_RADIUS = 4
TILE_Y, TILE_X = 32, 64  # kStencilTileY, kStencilTileX of csrc/kernels.h


def _parse_weights(weights):
    """``(r, taps)`` of a ``(2r+1, 2r+1)`` table; taps are ``(dy, dx,
    coefficient)`` in row-major order with the zero weights dropped."""
    k = torch.as_tensor(weights)
    if k.is_complex():
        raise TypeError("stencil weights must be real")
    k = k.detach().to("cpu", torch.float64)
    if k.dim() != 2 or k.shape[0] != k.shape[1] or k.shape[0] % 2 != 1:
        raise ValueError(
            f"weights must be a (2r+1, 2r+1) table, got shape "
            f"{tuple(k.shape)}")
    r = (k.shape[0] - 1) // 2
    if not 1 <= r <= MAX_RADIUS:
        raise ValueError(
            f"stencil radius must be in 1..{MAX_RADIUS}, got {r}")
    taps = []
    for a in range(2 * r + 1):
        for b in range(2 * r + 1):
            c = k[a, b].item()
            if c != 0.0:
                taps.append((a - r, b - r, c))
    if not taps:
        raise ValueError("a stencil needs at least one non-zero weight")
    return r, taps


def _span(t):
    lo = t.data_ptr()
    return lo, lo + t.numel() * t.element_size()


class HaloStencil:
    """See the module docstring.  Build with
    ``CartesianGrid.make_stencil``."""

    def __init__(self, grid, shape, dtype, device, weights, nfields=1,
                 _force_remote=False):
        if not isinstance(dtype, torch.dtype):
            raise TypeError(f"dtype must be a torch.dtype, got {dtype!r}")
        if dtype not in AD_DTYPES:
            raise TypeError(
                f"a halo stencil supports float16, bfloat16, float32 and "
                f"float64, got {dtype}")
        self._width, self._taps = _parse_weights(weights)
        self.exchanger = HaloExchanger(
            grid, shape, dtype, device, width=self._width, nfields=nfields,
            _force_remote=_force_remote)
        self.dtype = dtype
        self.acc_dtype = (torch.float64 if dtype == torch.float64
                          else torch.float32)
        self._tap_dy = [t[0] for t in self._taps]
        self._tap_dx = [t[1] for t in self._taps]
        self._tap_coef = [t[2] for t in self._taps]
        self._partials = None  # see _partials_buf

    @property
    def width(self):
        """The stencil's radius ``r``, which is the halo width."""
        return self._width

    @property
    def taps(self):
        """``[(dy, dx, coefficient), ...]`` in the order they are added."""
        return list(self._taps)

    # ------------------------------------------------------------------
    def _native(self):
        return (self.exchanger.device.type == "cuda"
                and not os.environ.get("MPI4JAX_AMD_HALO_PY"))

    def _outputs(self, ins, out, zero):
        ex = self.exchanger
        if out is None:
            make = torch.zeros if zero else torch.empty
            return [make(ex.shape, dtype=ex.dtype, device=ex.device)
                    for _ in ins]
        outs = [out] if isinstance(out, torch.Tensor) else list(out)
        ex._check(outs)
        spans = [_span(t) for t in list(ins) + outs]
        for k in range(len(ins), len(spans)):
            for j in range(k):
                if spans[k][0] < spans[j][1] and spans[j][0] < spans[k][1]:
                    raise ValueError(
                        f"out[{k - len(ins)}] overlaps "
                        + (f"input {j}" if j < len(ins)
                           else f"out[{j - len(ins)}]"))
        return outs

    def _ret(self, outs):
        return outs[0] if len(outs) == 1 else tuple(outs)

    def apply(self, *fields, out=None):
        """``A`` on ``fields``; the inputs (halos included) are never
        mutated.  With ``out=None`` the results are new tensors from
        ``torch.zeros`` with their interior filled: one tensor for one
        field, else a tuple.  ``out=`` takes one tensor or a sequence of
        ``nfields`` contiguous tensors of the exchanger's shape, dtype and
        device that overlap neither an input nor each other
        (``ValueError``); only their interior is written."""
        ex = self.exchanger
        ex._check(fields)
        outs = self._outputs(fields, out, zero=True)
        if self._native():
            self._call_native("halo_stencil_nd", fields, outs)
        else:
            self._apply_py(fields, outs)
        return self._ret(outs)

    def apply_ad(self, *fields):
        """Differentiable ``apply``: the same values, and a backward pass
        that runs :meth:`adjoint` on the incoming gradients.  Fields may
        require grad.  The backward pass is a collective and is once
        differentiable."""
        self.exchanger._check(fields, allow_grad=True)
        out = _StencilAD.apply(self, *fields)
        return out[0] if len(out) == 1 else out

    def adjoint(self, *gouts, out=None):
        """``A^T`` on ``gouts`` (gradients with respect to the outputs of
        ``apply``); the inputs are never mutated.  Returns the gradients
        with respect to the inputs of ``apply``, every cell written.
        ``out=`` as in :meth:`apply`.  A collective, like the exchange."""
        ex = self.exchanger
        ex._check(gouts)
        gins = self._outputs(gouts, out, zero=False)
        if self._native():
            if ex._adj_work >= 1 << 31:
                raise ValueError(
                    f"halo adjoint over {ex._adj_work} frame cells "
                    f"exceeds the native executor's 2^31 limit")
            self._call_native("halo_stencil_adjoint_nd", gouts, gins)
        else:
            self._adjoint_py(gouts, gins)
        return self._ret(gins)

    # ------------------------------------------------- inner products
    def _field_list(self, a):
        fields = (a,) if isinstance(a, torch.Tensor) else tuple(a)
        self.exchanger._check(fields)
        return fields

    def _scalar(self):
        return torch.empty((), dtype=torch.float64,
                           device=self.exchanger.device)

    def _partials_buf(self):
        """One float64 slot per block of the native kernels' tile grid
        (32 x 64 tiles of the interior of every plane), allocated once."""
        if self._partials is None:
            ex = self.exchanger
            w = self._width
            tiles = (-(-(ex.ny - 2 * w) // TILE_Y)
                     * -(-(ex.nx - 2 * w) // TILE_X))
            self._partials = torch.empty(
                ex.nfields * ex.levels * tiles, dtype=torch.float64,
                device=ex.device)
        return self._partials

    def _allreduce_(self, scalar):
        """Sum a local float64 scalar over the grid's communicator, in
        place, on the current stream.  One rank with nothing remote: no
        communicator is touched."""
        ex = self.exchanger
        if ex.comm.size > 1 or ex._has_remote:
            from ..ops.allreduce import allreduce
            from ..ops.reduce_ops import Op

            scalar.copy_(allreduce(scalar, Op.SUM, comm=ex.comm))
        return scalar

    def _interior(self, t):
        ex = self.exchanger
        w = self._width
        return t.view(ex.levels, ex.ny, ex.nx)[:, w:ex.ny - w, w:ex.nx - w]

    def _dot_into(self, a, b, result):
        """``result`` <- the global interior inner product of two checked
        field lists."""
        if self._native():
            from .._backend import rccl

            ex = self.exchanger
            rccl.ext().halo_interior_dot_nd(
                list(a), list(b), ex.levels, ex.ny, ex.nx, self._width,
                self._partials_buf(), result)
        else:
            total = None
            for fa, fb in zip(a, b):
                s = (self._interior(fa).double()
                     * self._interior(fb).double()).sum()
                total = s if total is None else total + s
            result.copy_(total)
        return self._allreduce_(result)

    def dot(self, a, b):
        """The inner product of ``a`` and ``b`` over the interior cells of
        every level of every field and over every rank of the grid: a 0-d
        float64 tensor on the fields' device.  ``a`` and ``b`` are each
        one tensor or a sequence of ``nfields`` tensors; halo cells do not
        count.  Every term is ``double(a[c]) * double(b[c])`` and all sums
        are float64, whatever the field dtype.  The native executor adds
        in one fixed order with no atomics (``csrc/krylov.hip``), so two
        runs agree bitwise; with more than one rank the local results go
        through ``allreduce(SUM)`` on the current stream, which makes this
        a collective."""
        a, b = self._field_list(a), self._field_list(b)
        return self._dot_into(a, b, self._scalar())

    def _apply_dot_into(self, fields, outs, result):
        if self._native():
            from .._backend import rccl

            ex = self.exchanger
            comm_id = rccl._handle(ex.comm) if ex._has_remote else -1
            rccl.ext().halo_stencil_dot_nd(
                list(fields), list(outs), ex.levels, ex.ny, ex.nx,
                self._width, self._tap_dy, self._tap_dx, self._tap_coef,
                ex._send_to, ex._recv_from, ex._local_mask, ex._sbuf,
                ex._rbuf, comm_id, self._partials_buf(), result)
            return self._allreduce_(result)
        self._apply_py(fields, outs)
        return self._dot_into(fields, outs, result)

    def apply_dot(self, *fields, out=None):
        """``(out, pAp)``: ``out`` is exactly what :meth:`apply` returns,
        bit for bit, and ``pAp`` is ``dot(fields, out)``, the product taken
        with the outputs as stored.  The native executor forms the local
        sum in the stencil launch itself, followed by one small finish
        launch."""
        ex = self.exchanger
        ex._check(fields)
        outs = self._outputs(fields, out, zero=True)
        pap = self._apply_dot_into(fields, outs, self._scalar())
        return self._ret(outs), pap

    def make_cg(self):
        """A :class:`~.cg.StencilCG`: conjugate gradients for ``A x = b``
        with this operator.  float32 and float64 only (``TypeError``)."""
        from .cg import StencilCG

        return StencilCG(self)

    def gershgorin_bounds(self):
        """``(centre - s, centre + s)`` as floats, ``s`` the sum of the
        magnitudes of the off-centre weights: Gershgorin's interval for
        the eigenvalues of ``A`` on interior vectors.  It is rigorous for
        symmetric weights whatever the edges: on a fully periodic grid
        every row of ``A`` holds exactly these weights, and closed edges
        with a zero halo leave a principal submatrix of that matrix,
        whose eigenvalues lie between the same bounds (and decomposed
        edges do not change the global matrix).  The lower bound is only
        useful when it is positive, that is for a diagonally dominant
        stencil such as ``I - nu * lap``."""
        centre = sum(c for dy, dx, c in self._taps if dy == 0 and dx == 0)
        s = sum(abs(c) for dy, dx, c in self._taps if dy != 0 or dx != 0)
        return float(centre - s), float(centre + s)

    def make_chebyshev(self, lmin, lmax):
        """A :class:`~.chebyshev.StencilChebyshev`: Chebyshev iteration
        for ``A x = b`` given ``0 < lmin <= lambda(A) <= lmax``
        (``ValueError`` unless ``0 < lmin < lmax < inf``; nothing checks
        that the bounds hold).  float32 and float64 only
        (``TypeError``)."""
        from .chebyshev import StencilChebyshev

        return StencilChebyshev(self, lmin, lmax)

    # ------------------------------------------------------------------
    def _call_native(self, entry, ins, outs):
        from .._backend import rccl

        ex = self.exchanger
        comm_id = rccl._handle(ex.comm) if ex._has_remote else -1
        getattr(rccl.ext(), entry)(
            list(ins), list(outs), ex.levels, ex.ny, ex.nx, self._width,
            self._tap_dy, self._tap_dx, self._tap_coef, ex._send_to,
            ex._recv_from, ex._local_mask, ex._sbuf, ex._rbuf, comm_id)

    def _apply_py(self, fields, outs):
        ex = self.exchanger
        L, ny, nx, w = ex.levels, ex.ny, ex.nx, self._width
        exchanged = ex.exchange(*fields)
        if isinstance(exchanged, torch.Tensor):
            exchanged = (exchanged,)
        for e, o in zip(exchanged, outs):
            v = e.view(L, ny, nx).to(self.acc_dtype)
            acc = torch.zeros(L, ny - 2 * w, nx - 2 * w,
                              dtype=self.acc_dtype, device=e.device)
            for dy, dx, c in self._taps:
                acc += c * v[:, w + dy:ny - w + dy, w + dx:nx - w + dx]
            o.view(L, ny, nx)[:, w:ny - w, w:nx - w].copy_(acc)

    def _adjoint_py(self, gouts, gins):
        ex = self.exchanger
        L, ny, nx, w = ex.levels, ex.ny, ex.nx, self._width
        for g, o in zip(gouts, gins):
            src = g.view(L, ny, nx)[:, w:ny - w, w:nx - w].to(self.acc_dtype)
            acc = torch.zeros(L, ny, nx, dtype=self.acc_dtype,
                              device=g.device)
            for dy, dx, c in self._taps:
                acc[:, w + dy:ny - w + dy, w + dx:nx - w + dx] += c * src
            o.view(L, ny, nx).copy_(acc)
        ex.adjoint_(*gins)


class _StencilAD(torch.autograd.Function):
    """``HaloStencil.apply_ad``: forward = ``apply``, backward =
    ``adjoint`` on contiguous copies of the gradients."""

    @staticmethod
    def forward(ctx, st, *fields):
        ctx.st = st
        out = st.apply(*(f.detach() for f in fields))
        return out if isinstance(out, tuple) else (out,)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        # gradients of unused outputs arrive materialised as zeros; every
        # rank runs the same collective whatever its loss looks at
        gout = tuple(g.detach().contiguous() for g in grads)
        gin = ctx.st.adjoint(*gout)
        if isinstance(gin, torch.Tensor):
            gin = (gin,)
        return (None,) + tuple(
            g if need else None
            for g, need in zip(gin, ctx.needs_input_grad[1:]))
