"""Reusable halo exchanger: wide halos, batch dims, many fields.

``CartesianGrid.halo_exchange`` refreshes the 1-cell ring of one 2-D
array.  A :class:`HaloExchanger` (built by
``CartesianGrid.make_halo_exchanger``) does the same job for user stencil
codes: fields of shape ``(..., ny, nx)`` whose leading dimensions are batch
"levels", a halo of ``width`` cells, and up to eight fields exchanged
together.  It owns its staging buffers and its resolved schedule, both
built once.

Semantics (they generalise :func:`..parallel.grid.halo_plan`):

* **Reads.**  Every outgoing strip is read from the pre-exchange state.
* **Writes** land in the order columns, rows, corners.
* **Columns.**  The ``width``-wide interior strip next to the west / east
  edge goes to that neighbour's opposite halo strip, over the FULL height
  (halo rows included).
* **Rows.**  The ``width``-high interior strip next to the south / north
  edge goes to that neighbour's opposite halo strip, over the interior
  columns ``[width, nx - width)`` only.
* **Corners.**  The ``width`` x ``width`` interior corner block goes to the
  diagonal neighbour's opposite halo corner block and wins over what a
  column strip wrote there.
* **Closed edges.**  Halo cells with no sender keep their values.

At ``width=1`` on one 2-D field the result is bitwise equal to
``CartesianGrid.halo_exchange``.

Matching is by enqueue order, not by tag.  The eight directions come in
the fixed order :data:`DIRECTIONS`; entry *i* pairs "send toward d_i" with
"receive from -d_i", and there is exactly one message per direction
carrying all fields and all levels as ``[field][level][row][col]``.  Two
ranks that are neighbours in more than one direction (a 1x2 periodic grid)
therefore still pair up.

Executors:

* the **native** executor (default on the GPU) is one call into
  ``csrc/bridge.cpp:halo_exchange_nd``: one pack launch, one RCCL group,
  one unpack launch.  Self-peer strips (periodic wraps on an undecomposed
  axis) are packed straight into the receive staging buffer, so an exchange
  with no remote peer never touches RCCL and is capturable in a
  ``torch.cuda.graph``;
* the **Python** executor (any device; the CPU path; forced on the GPU by
  ``MPI4JAX_AMD_HALO_PY=1``) packs with torch slicing and issues one
  ``sendrecv`` / ``send`` / ``recv`` per schedule entry — the same message
  sizes in the same order.

Autodiff.  ``exchange`` and ``exchange_`` are NOT differentiable (they
mutate staging buffers and, for ``exchange_``, the fields) and reject a
field that requires grad.  ``exchange_ad`` is the differentiable
out-of-place exchange: same values as ``exchange``, with a backward pass
that runs the exchange's adjoint.  The adjoint is also public as
``adjoint`` / ``adjoint_`` for adjoint-method solvers that call it
directly.  Floating dtypes only (float16, bfloat16, float32, float64).

The forward exchange is a gather — every output cell reads exactly one
pre-exchange cell, a sender's source cell or itself — so the adjoint is a
scatter-add with the message directions reversed:

1. the RECEIVE window of every entry that has a receiver is packed into
   slot *i* (for a column entry, the corner rows that a present corner
   entry owned in the forward pass are packed as zeros);
2. slot *i* is sent to ``recv_from[i]`` and received from ``send_to[i]``,
   in the same fixed entry order;
3. every receive window that has a receiver is zeroed (the forward pass
   overwrote those cells, so nothing flows through them), and received
   slot *i* is added into the SEND window of entry *i*.

Send windows overlap (a column strip is full height; rows and corner
blocks lie inside it), so one cell collects up to 9 terms.  Every executor
forms that sum in the same order — the cell's own value (or 0 if it was
overwritten), then the received terms in REVERSE :data:`DIRECTIONS` order
(corners, S, N, E, W) — float32 / float64 in their own precision, float16
/ bfloat16 in float32 with one rounding at the store.  The executors
therefore agree bitwise.  The reverse order is the one reverse-mode
autodiff uses on the forward pass's sequence of writes, so at ``width=1``
the gradient is bitwise that of autograd through
``CartesianGrid.halo_exchange``.
A halo cell at a closed edge has no sender: the forward pass keeps it, and
its gradient passes straight through.

**The backward pass is a collective.**  Every rank must run it, and the
exchanges must be differentiated in the reverse of their forward order.
Both follow automatically when every rank runs the same program and every
rank's loss depends on its exchanged fields; a rank that skips
``backward()`` (or an ``exchange_ad`` none of whose inputs requires grad
on one rank only) leaves its neighbours waiting.  Use
``CartesianGrid.halo_exchange`` when a one-cell, one-field exchange
composed of ``sendrecv`` is all that is needed.
"""

import os

import torch
from torch.autograd.function import once_differentiable

# (dy, dx); y grows northward, x eastward (CartesianGrid convention).
# Columns (W, E), rows (N, S), corners — the order of grid.halo_plan.
DIRECTIONS = (
    (0, -1), (0, 1),
    (1, 0), (-1, 0),
    (-1, -1), (-1, 1), (1, -1), (1, 1),
)

MAX_FIELDS = 8

# dtypes of exchange_ad and the adjoint (the accumulate step is arithmetic)
AD_DTYPES = (torch.float16, torch.bfloat16, torch.float32, torch.float64)


def _axis(d, n, w, full):
    """(send_start, recv_start, length) along one axis for direction
    component ``d``.  ``d == 0`` spans the whole axis (``full``: column
    strips run over the halo rows too) or its interior (row strips)."""
    if d < 0:
        return w, n - w, w
    if d > 0:
        return n - 2 * w, 0, w
    if full:
        return 0, 0, n
    return w, w, n - 2 * w


class HaloExchanger:
    """See the module docstring.  Build with
    ``CartesianGrid.make_halo_exchanger``."""

    def __init__(self, grid, shape, dtype, device, width=1, nfields=1,
                 _force_remote=False):
        if isinstance(width, bool) or not isinstance(width, int):
            raise TypeError(f"width must be an int, got {type(width)}")
        if isinstance(nfields, bool) or not isinstance(nfields, int):
            raise TypeError(f"nfields must be an int, got {type(nfields)}")
        if not isinstance(dtype, torch.dtype):
            raise TypeError(f"dtype must be a torch.dtype, got {dtype!r}")
        if width < 1:
            raise ValueError(f"halo width must be >= 1, got {width}")
        if not 1 <= nfields <= MAX_FIELDS:
            raise ValueError(
                f"nfields must be in 1..{MAX_FIELDS}, got {nfields}")
        shape = tuple(int(s) for s in shape)
        if len(shape) < 2:
            raise ValueError(
                f"shape must be (..., ny, nx) with at least 2 dims, "
                f"got {shape}")
        ny, nx = shape[-2:]
        if ny < 3 * width or nx < 3 * width:
            raise ValueError(
                f"each decomposed axis needs n >= 3*width so that every "
                f"strip is read from true interior cells; got (ny, nx) = "
                f"({ny}, {nx}) with width {width}")
        levels = 1
        for s in shape[:-2]:
            levels *= s
        if levels < 1:
            raise ValueError(f"empty batch dimensions in shape {shape}")
        self.grid = grid
        self.comm = grid.comm
        self.shape = shape
        self.dtype = dtype
        self.device = torch.device(device)
        self.width = width
        self.nfields = nfields
        self.levels = levels
        self.ny, self.nx = ny, nx
        self._force_remote = bool(_force_remote)
        self._esz = torch.empty(0, dtype=dtype).element_size()
        if self.device.type == "cuda" and self._esz not in (1, 2, 4, 8):
            raise TypeError(
                f"the GPU halo exchanger moves 1/2/4/8-byte elements; "
                f"{dtype} has {self._esz}")

        # resolved schedule: one entry per direction, fixed order
        me = self.comm.rank
        w = width
        self._entries = []
        off = 0
        for i, (dy, dx) in enumerate(DIRECTIONS):
            sy, ry, h = _axis(dy, ny, w, full=True)
            sx, rx, wd = _axis(dx, nx, w, full=False)
            n = nfields * levels * h * wd
            st = grid.neighbor2(dy, dx)
            rf = grid.neighbor2(-dy, -dx)
            local = (st == me and rf == me and not self._force_remote)
            self._entries.append(dict(
                index=i, direction=(dy, dx), send_to=st, recv_from=rf,
                local=local, n=n, off=off, h=h, wd=wd,
                send=(sy, sx), recv=(ry, rx)))
            off += n
        self._total = off
        self._send_to = [-1 if e["send_to"] is None else int(e["send_to"])
                         for e in self._entries]
        self._recv_from = [
            -1 if e["recv_from"] is None else int(e["recv_from"])
            for e in self._entries]
        self._local_mask = sum(1 << e["index"] for e in self._entries
                               if e["local"])
        self._has_remote = any(
            not e["local"] and (e["send_to"] is not None
                                or e["recv_from"] is not None)
            for e in self._entries)
        if self.device.type == "cuda" and off >= 1 << 31:
            raise ValueError(
                f"halo staging of {off} elements exceeds the native "
                f"executor's 2^31 limit")
        self._sbuf = torch.empty(off, dtype=dtype, device=self.device)
        self._rbuf = torch.empty(off, dtype=dtype, device=self.device)
        # work items of the native adjoint's accumulate kernel: one per
        # cell of the 2*width-thick frame (the whole level when an axis
        # is shorter than 4*width); checked when the adjoint is called.
        # The same formula as halo_frame() in csrc/halo_geom.h, which
        # halo_adjoint_nd checks again: change the two together.
        if ny < 4 * w or nx < 4 * w:
            frame = ny * nx
        else:
            frame = 4 * w * nx + (ny - 4 * w) * 4 * w
        self._adj_work = nfields * levels * frame

    # ------------------------------------------------------------------
    @property
    def local_directions(self):
        """Directions executed as local copies (self-peer periodic wraps);
        they never reach the communicator."""
        return tuple(e["direction"] for e in self._entries if e["local"])

    def schedule(self):
        """``[(direction, send_to, recv_from, n_elements), ...]`` in
        enqueue order; ranks are comm-relative, ``None`` = no peer.
        Entries with no peer at all are omitted.  Entries whose direction
        is in :attr:`local_directions` are local copies."""
        return [(e["direction"], e["send_to"], e["recv_from"], e["n"])
                for e in self._entries
                if e["send_to"] is not None or e["recv_from"] is not None]

    def adjoint_schedule(self):
        """The mirror of :meth:`schedule` for :meth:`adjoint_`: the same
        entries in the same order with the roles swapped — the adjoint
        sends slot *i* to the forward pass's ``recv_from`` and receives it
        from the forward pass's ``send_to``."""
        return [(e["direction"], e["recv_from"], e["send_to"], e["n"])
                for e in self._entries
                if e["send_to"] is not None or e["recv_from"] is not None]

    # ------------------------------------------------------------------
    def _check(self, fields, allow_grad=False):
        if len(fields) != self.nfields:
            raise ValueError(
                f"exchanger was built for {self.nfields} field(s), got "
                f"{len(fields)}")
        for k, f in enumerate(fields):
            if not isinstance(f, torch.Tensor):
                raise TypeError(
                    f"field {k} must be a torch.Tensor, got {type(f)}")
            if tuple(f.shape) != self.shape:
                raise ValueError(
                    f"field {k} has shape {tuple(f.shape)}, exchanger was "
                    f"built for {self.shape}")
            if f.dtype != self.dtype:
                raise TypeError(
                    f"field {k} has dtype {f.dtype}, exchanger was built "
                    f"for {self.dtype}")
            if f.device != self._sbuf.device:
                raise ValueError(
                    f"field {k} lives on {f.device}, exchanger was built "
                    f"for {self._sbuf.device}")
            if not f.is_contiguous():
                raise ValueError(f"field {k} must be contiguous")
            if f.requires_grad and not allow_grad:
                # exchange / exchange_ / adjoint / adjoint_ mutate in
                # place; exchange_ad is the differentiable entry
                raise ValueError(
                    f"field {k} requires grad: the halo exchanger is not "
                    f"differentiable — use CartesianGrid.halo_exchange "
                    f"under autograd, or HaloExchanger.exchange_ad")

    def _check_ad_dtype(self, what):
        if self.dtype not in AD_DTYPES:
            raise TypeError(
                f"{what} supports float16, bfloat16, float32 and float64; "
                f"this exchanger was built for {self.dtype}")

    def exchange(self, *fields):
        """Exchange copies of ``fields``; the inputs are never mutated.
        Returns one new tensor for one field, else a tuple."""
        self._check(fields)
        return self.exchange_(*(f.clone() for f in fields))

    def exchange_(self, *fields):
        """In-place exchange.  Returns the field (one) or the tuple of
        fields it was given."""
        self._check(fields)
        if (self.device.type == "cuda"
                and not os.environ.get("MPI4JAX_AMD_HALO_PY")):
            self._exchange_native(fields)
        else:
            self._exchange_py(fields)
        return fields[0] if len(fields) == 1 else fields

    def exchange_ad(self, *fields):
        """Differentiable out-of-place exchange: the values of
        :meth:`exchange`, and a backward pass that runs :meth:`adjoint_`
        on the incoming gradients.  Fields may require grad.  The backward
        pass is a collective (see the module docstring) and is once
        differentiable."""
        self._check_ad_dtype("exchange_ad")
        self._check(fields, allow_grad=True)
        out = _ExchangeAD.apply(self, *fields)
        return out[0] if len(out) == 1 else out

    def adjoint(self, *grads):
        """Adjoint of the exchange on copies of ``grads`` (gradients with
        respect to the exchange's outputs); the inputs are never mutated.
        Returns the gradients with respect to the exchange's inputs: one
        new tensor for one field, else a tuple."""
        self._check_ad_dtype("adjoint")
        self._check(grads)
        return self.adjoint_(*(g.clone() for g in grads))

    def adjoint_(self, *grads):
        """In-place adjoint.  Returns the gradient (one) or the tuple of
        gradients it was given.  A collective, like the exchange."""
        self._check_ad_dtype("adjoint_")
        self._check(grads)
        if (self.device.type == "cuda"
                and not os.environ.get("MPI4JAX_AMD_HALO_PY")):
            if self._adj_work >= 1 << 31:
                raise ValueError(
                    f"halo adjoint over {self._adj_work} frame cells "
                    f"exceeds the native executor's 2^31 limit")
            self._adjoint_native(grads)
        else:
            self._adjoint_py(grads)
        return grads[0] if len(grads) == 1 else grads

    # ------------------------------------------------------------------
    def _adjoint_native(self, grads):
        from .._backend import rccl

        comm_id = rccl._handle(self.comm) if self._has_remote else -1
        rccl.ext().halo_adjoint_nd(
            list(grads), self.levels, self.ny, self.nx, self.width,
            self._send_to, self._recv_from, self._local_mask,
            self._sbuf, self._rbuf, comm_id)

    def _adjoint_py(self, grads):
        from ..ops.sendrecv import sendrecv
        from ..ops.send import send
        from ..ops.recv import recv

        L, ny, nx, nf = self.levels, self.ny, self.nx, self.nfields
        w = self.width
        views = [g.view(L, ny, nx) for g in grads]
        ents = self._entries

        def slot(buf, e):
            return buf[e["off"]:e["off"] + e["n"]].view(
                nf, L, e["h"], e["wd"])

        # adjoint pack: receive windows, read before anything is written.
        # The corner rows of a column slot that a corner entry owned in
        # the forward pass were never written from this slot: zeros.
        for e in ents:
            if e["recv_from"] is None:
                continue
            y0, x0 = e["recv"]
            dst = slot(self._rbuf if e["local"] else self._sbuf, e)
            for k, v in enumerate(views):
                dst[k].copy_(v[:, y0:y0 + e["h"], x0:x0 + e["wd"]])
            if e["index"] < 2:
                lo, hi = (6, 4) if e["index"] == 0 else (7, 5)
                if ents[lo]["recv_from"] is not None:
                    dst[:, :, :w].zero_()
                if ents[hi]["recv_from"] is not None:
                    dst[:, :, e["h"] - w:].zero_()

        # one message per direction, fixed order, roles swapped
        me = self.comm.rank
        for e in ents:
            st, rf = e["recv_from"], e["send_to"]
            if e["local"] or (st is None and rf is None):
                continue
            sview = slot(self._sbuf, e)
            rview = slot(self._rbuf, e)
            if st == me and rf == me:
                rview.copy_(sview)
            elif st is None:
                rview.copy_(recv(rview, source=rf, comm=self.comm))
            elif rf is None:
                send(sview, dest=st, comm=self.comm)
            else:
                rview.copy_(sendrecv(sview, rview, source=rf, dest=st,
                                     comm=self.comm))

        # accumulate: own value (0 where the forward pass overwrote the
        # cell), then the received terms in REVERSE entry order; the half
        # types sum on a float32 copy and round once
        half = self.dtype in (torch.float16, torch.bfloat16)
        acc = [v.float() for v in views] if half else views
        for e in ents:
            if e["recv_from"] is None:
                continue
            y0, x0 = e["recv"]
            for a in acc:
                a[:, y0:y0 + e["h"], x0:x0 + e["wd"]].zero_()
        for e in reversed(ents):
            if e["send_to"] is None:
                continue
            y0, x0 = e["send"]
            src = slot(self._rbuf, e)
            for k, a in enumerate(acc):
                a[:, y0:y0 + e["h"], x0:x0 + e["wd"]] += (
                    src[k].float() if half else src[k])
        if half:
            for v, a in zip(views, acc):
                v.copy_(a)

    def _exchange_native(self, fields):
        from .._backend import rccl

        # comm lookup (and the lazy RCCL init behind it) only when some
        # strip really leaves this rank
        comm_id = rccl._handle(self.comm) if self._has_remote else -1
        rccl.ext().halo_exchange_nd(
            list(fields), self.levels, self.ny, self.nx, self.width,
            self._send_to, self._recv_from, self._local_mask,
            self._sbuf, self._rbuf, comm_id)

    def _exchange_py(self, fields):
        # imported here to avoid a circular import at package init
        from ..ops.sendrecv import sendrecv
        from ..ops.send import send
        from ..ops.recv import recv

        L, ny, nx, nf = self.levels, self.ny, self.nx, self.nfields
        views = [f.view(L, ny, nx) for f in fields]

        def slot(buf, e):
            return buf[e["off"]:e["off"] + e["n"]].view(
                nf, L, e["h"], e["wd"])

        # pack: every strip is read before anything is written.  Self-peer
        # strips go straight into the receive staging slot.
        for e in self._entries:
            if e["send_to"] is None:
                continue
            y0, x0 = e["send"]
            dst = slot(self._rbuf if e["local"] else self._sbuf, e)
            for k, v in enumerate(views):
                dst[k].copy_(v[:, y0:y0 + e["h"], x0:x0 + e["wd"]])

        # one message per direction, fixed order
        me = self.comm.rank
        for e in self._entries:
            st, rf = e["send_to"], e["recv_from"]
            if e["local"] or (st is None and rf is None):
                continue
            sview = slot(self._sbuf, e)
            rview = slot(self._rbuf, e)
            if st == me and rf == me:
                # _force_remote at the op layer: self p2p is a local copy
                rview.copy_(sview)
            elif st is None:
                rview.copy_(recv(rview, source=rf, comm=self.comm))
            elif rf is None:
                send(sview, dest=st, comm=self.comm)
            else:
                rview.copy_(sendrecv(sview, rview, source=rf, dest=st,
                                     comm=self.comm))

        # unpack in entry order: columns, rows, corners (corners win)
        for e in self._entries:
            if e["recv_from"] is None:
                continue
            y0, x0 = e["recv"]
            src = slot(self._rbuf, e)
            for k, v in enumerate(views):
                v[:, y0:y0 + e["h"], x0:x0 + e["wd"]].copy_(src[k])


class _ExchangeAD(torch.autograd.Function):
    """``HaloExchanger.exchange_ad``: forward = ``exchange_`` on clones,
    backward = ``adjoint_`` on contiguous clones of the gradients."""

    @staticmethod
    def forward(ctx, ex, *fields):
        ctx.ex = ex
        out = tuple(f.detach().clone() for f in fields)
        ex.exchange_(*out)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        # gradients of unused outputs arrive materialised as zeros; every
        # rank runs the same collective whatever its loss looks at
        gin = tuple(g.detach().clone(memory_format=torch.contiguous_format)
                    for g in grads)
        ctx.ex.adjoint_(*gin)
        return (None,) + tuple(
            g if need else None
            for g, need in zip(gin, ctx.needs_input_grad[1:]))
