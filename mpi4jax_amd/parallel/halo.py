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

The exchanger is NOT differentiable (it mutates staging buffers and, for
``exchange_``, the fields); use ``CartesianGrid.halo_exchange`` under
autograd.
"""

import os

import torch

# (dy, dx); y grows northward, x eastward (CartesianGrid convention).
# Columns (W, E), rows (N, S), corners — the order of grid.halo_plan.
DIRECTIONS = (
    (0, -1), (0, 1),
    (1, 0), (-1, 0),
    (-1, -1), (-1, 1), (1, -1), (1, 1),
)

MAX_FIELDS = 8


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

    # ------------------------------------------------------------------
    def _check(self, fields):
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
            if f.requires_grad:
                raise ValueError(
                    f"field {k} requires grad: the halo exchanger is not "
                    f"differentiable — use CartesianGrid.halo_exchange "
                    f"under autograd")

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

    # ------------------------------------------------------------------
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
