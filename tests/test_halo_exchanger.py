"""CPU suite for parallel/halo.HaloExchanger (wide halos, batch dims,
many fields).  Every comparison is bitwise: an exchange only copies.

The oracle works on a global array whose values encode
(field, level, global j, global i).  Each rank takes its block with halos
pre-filled by one common sentinel; expected halos come from the global
array with wrap-around where the grid is periodic (or a neighbour
exists), and the sentinel stays at closed edges — including the corner
blocks a full-height column strip carries from a neighbour's halo rows,
which are sentinel too.
"""

import itertools
import os
import subprocess
import sys

import pytest
import torch

import mpi4jax_amd as m
from mpi4jax_amd.parallel.grid import CartesianGrid
from _mp import run_multiproc

PERIODIC = [(True, True), (False, True), (True, False), (False, False)]


# ------------------------------------------------------------------ oracle

def cast(a, dtype):
    """int64 ids -> dtype, exactly representable in every dtype used."""
    if dtype in (torch.float64, torch.float32, torch.int64):
        return a.to(dtype)  # ids stay far below 2^24
    if dtype == torch.bool:
        return (a % 251) % 2 == 1
    return (a % 251).to(dtype)  # uint8, bfloat16: exact below 256


def sentinel(dtype):
    return cast(torch.tensor(-7 if dtype != torch.uint8 else 253), dtype)


def global_ids(nf, levels, gy, gx):
    """(nf, levels, gy, gx) int64: a distinct id per (f, l, j, i)."""
    return torch.arange(nf * levels * gy * gx, dtype=torch.int64).reshape(
        nf, levels, gy, gx)


def local_fields(G, dims, coords, w, dtype, batch):
    """This rank's blocks of G with sentinel halos: list of nf tensors of
    shape batch + (by + 2w, bx + 2w)."""
    nf, levels, gy, gx = G.shape
    by, bx = gy // dims[0], gx // dims[1]
    cy, cx = coords
    out = []
    for f in range(nf):
        a = sentinel(dtype).expand(levels, by + 2 * w, bx + 2 * w).clone()
        a[:, w:w + by, w:w + bx] = cast(
            G[f, :, cy * by:(cy + 1) * by, cx * bx:(cx + 1) * bx], dtype)
        out.append(a.reshape(tuple(batch) + (by + 2 * w, bx + 2 * w)))
    return out


def expected_fields(G, dims, coords, periodic, w, dtype, batch):
    nf, levels, gy, gx = G.shape
    by, bx = gy // dims[0], gx // dims[1]
    cy, cx = coords
    gj = cy * by + torch.arange(by + 2 * w) - w
    gi = cx * bx + torch.arange(bx + 2 * w) - w
    ok_y = ((gj >= 0) & (gj < gy)) | bool(periodic[0])
    ok_x = ((gi >= 0) & (gi < gx)) | bool(periodic[1])
    gj, gi = gj % gy, gi % gx
    mask = ok_y[:, None] & ok_x[None, :]
    out = []
    for f in range(nf):
        e = cast(G[f][:, gj[:, None], gi[None, :]], dtype)
        e = torch.where(mask, e, sentinel(dtype))
        out.append(e.reshape(tuple(batch) + (by + 2 * w, bx + 2 * w)))
    return out


class FakeComm:
    def __init__(self, rank, size):
        self.rank, self.size = rank, size

    def rccl_handle(self):
        return 1000 + self.rank  # never dereferenced on the CPU


def fake_grid(rank, dims, periodic):
    g = CartesianGrid.__new__(CartesianGrid)
    g.comm = FakeComm(rank, dims[0] * dims[1])
    g.nproc_y, g.nproc_x = dims
    g.periodic_y, g.periodic_x = periodic
    g.coords = (rank // dims[1], rank % dims[1])
    return g


def world1_case(shape, w, nf, dtype, periodic, device="cpu"):
    """(fields, expected) for a 1x1 grid; `shape` includes the halo."""
    batch = shape[:-2]
    levels = 1
    for s in batch:
        levels *= s
    G = global_ids(nf, levels, shape[-2] - 2 * w, shape[-1] - 2 * w)
    fields = local_fields(G, (1, 1), (0, 0), w, dtype, batch)
    exp = expected_fields(G, (1, 1), (0, 0), periodic, w, dtype, batch)
    return ([f.to(device) for f in fields], [e.to(device) for e in exp])


# ----------------------------------------------------------------- world 1

@pytest.fixture(scope="module")
def grids():
    m.init()
    return {p: CartesianGrid(dims=(1, 1), periodic=p) for p in PERIODIC}


def _shapes(w):
    return [(3 * w, 3 * w), (37, 53), (5, 11, 13), (2, 3, 9, 10)]


@pytest.mark.parametrize("periodic", PERIODIC)
@pytest.mark.parametrize("w", [1, 2, 3])
@pytest.mark.parametrize("shape_idx", range(4))
def test_world1_matches_oracle(grids, periodic, w, shape_idx):
    shape = _shapes(w)[shape_idx]
    grid = grids[periodic]
    for nf in (1, 3, 8):
        for dtype in (torch.float64, torch.float32, torch.int64,
                      torch.uint8, torch.bool):
            fields, exp = world1_case(shape, w, nf, dtype, periodic)
            orig = [f.clone() for f in fields]
            ex = grid.make_halo_exchanger(shape, dtype, "cpu", width=w,
                                          nfields=nf)
            out = ex.exchange(*fields)
            out = (out,) if nf == 1 else out
            inner = (Ellipsis, slice(w, -w), slice(w, -w))
            for f, o, e, x in zip(fields, out, exp, orig):
                assert torch.equal(f, x), "exchange() mutated its input"
                assert torch.equal(o, e), (shape, w, nf, dtype)
                assert torch.equal(o[inner], x[inner])
                if periodic == (False, False):
                    assert torch.equal(o, x)
            # in-place form: same result, returns the fields themselves
            ret = ex.exchange_(*fields)
            ret = (ret,) if nf == 1 else ret
            for f, r, e in zip(fields, ret, exp):
                assert r is f
                assert torch.equal(f, e)


def test_world1_width1_equals_halo_exchange(grids):
    torch.manual_seed(3)
    for periodic in PERIODIC:
        grid = grids[periodic]
        a = torch.randn(37, 53, dtype=torch.float64)  # random halos too
        ex = grid.make_halo_exchanger(a.shape, a.dtype, "cpu")
        assert torch.equal(ex.exchange(a), grid.halo_exchange(a))


# --------------------------------------------------------- worlds 2 and 4

DIMS = {2: [(2, 1), (1, 2)], 4: [(2, 2), (1, 4), (4, 1)]}


def _multirank(rank, ws):
    comm = m.get_world()
    for dims, periodic, w in itertools.product(DIMS[ws], PERIODIC, (1, 2)):
        grid = CartesianGrid(comm=comm, dims=dims, periodic=periodic)
        batch, nf, dtype = (3,), 2, torch.float64
        G = global_ids(nf, 3, 6 * dims[0], 8 * dims[1])
        fields = local_fields(G, dims, grid.coords, w, dtype, batch)
        exp = expected_fields(G, dims, grid.coords, periodic, w, dtype,
                              batch)
        ex = grid.make_halo_exchanger(fields[0].shape, dtype, "cpu",
                                      width=w, nfields=nf)
        ex.exchange_(*fields)
        for f, e in zip(fields, exp):
            assert torch.equal(f, e), (dims, periodic, w, rank)
        if w == 1:
            torch.manual_seed(100 + rank)
            a = torch.randn(9, 11, dtype=torch.float64)
            ex1 = grid.make_halo_exchanger(a.shape, a.dtype, "cpu")
            got = ex1.exchange(a)
            ref = grid.halo_exchange(a)
            assert torch.equal(got, ref), (dims, periodic, rank)


def _multirank_all(rank, ws):
    _multirank(rank, ws)
    _invariance(rank, ws)


@pytest.mark.parametrize("ws", [2, 4])
def test_multirank_oracle_halo_exchange_and_invariance(ws):
    """One spawn per world size (process start-up dominates the cost):
    the oracle and ``grid.halo_exchange`` comparisons, then decomposition
    invariance — k=3 rounds of exchange + width-2 stencil, after which
    every rank's block of the world-2/4 result equals the same block of
    the world-1 field bitwise."""
    run_multiproc(_multirank_all, ws)


# ------------------------------------------------ decomposition invariance

def _stencil_step(u, w=2):
    """Width-2 update touching the axis neighbours at distance 1 and 2 and
    the four distance-2 diagonals, so columns, rows AND corners matter.
    Pure elementwise torch ops: every cell sees the same arithmetic
    whatever block it lives in."""
    c = u[..., 2:-2, 2:-2]
    lap = ((-u[..., 2:-2, :-4] + 16.0 * u[..., 2:-2, 1:-3] - 30.0 * c
            + 16.0 * u[..., 2:-2, 3:-1] - u[..., 2:-2, 4:]) / 12.0
           + (-u[..., :-4, 2:-2] + 16.0 * u[..., 1:-3, 2:-2] - 30.0 * c
              + 16.0 * u[..., 3:-1, 2:-2] - u[..., 4:, 2:-2]) / 12.0)
    diag = (u[..., :-4, :-4] + u[..., :-4, 4:] + u[..., 4:, :-4]
            + u[..., 4:, 4:] - 4.0 * c)
    new = u.clone()
    new[..., 2:-2, 2:-2] = c + 0.05 * lap + 0.01 * diag
    return new


def _run_rounds(grid, dims, G, k=3):
    w = 2
    by, bx = G.shape[-2] // dims[0], G.shape[-1] // dims[1]
    cy, cx = grid.coords
    u = torch.zeros(G.shape[0], by + 4, bx + 4, dtype=torch.float64)
    u[:, w:-w, w:-w] = G[:, cy * by:(cy + 1) * by, cx * bx:(cx + 1) * bx]
    ex = grid.make_halo_exchanger(u.shape, u.dtype, "cpu", width=w)
    for _ in range(k):
        ex.exchange_(u)
        u = _stencil_step(u)
    return u[:, w:-w, w:-w]


def _invariance(rank, ws):
    comm = m.get_world()
    torch.manual_seed(11)  # same global field on every rank
    G = torch.randn(2, 24, 24, dtype=torch.float64)
    for periodic in PERIODIC:
        ref = _run_rounds(fake_grid(0, (1, 1), periodic), (1, 1), G)
        for dims in DIMS[ws]:
            grid = CartesianGrid(comm=comm, dims=dims, periodic=periodic)
            got = _run_rounds(grid, dims, G)
            by, bx = 24 // dims[0], 24 // dims[1]
            cy, cx = grid.coords
            mine = ref[:, cy * by:(cy + 1) * by, cx * bx:(cx + 1) * bx]
            assert torch.equal(got, mine), (dims, periodic, rank)


# -------------------------------------------- schedule matching, no procs

TOPOLOGIES = [(1, 1), (2, 1), (1, 2), (2, 2), (2, 4), (4, 2), (1, 8),
              (8, 1), (2, 3), (3, 2)]


@pytest.mark.parametrize("dims", TOPOLOGIES)
def test_schedule_cross_rank_matching(dims):
    size = dims[0] * dims[1]
    for periodic, w, nf, force in itertools.product(
            PERIODIC, (1, 3), (1, 3), (False, True)):
        sends, recvs = {}, {}
        for rank in range(size):
            ex = fake_grid(rank, dims, periodic).make_halo_exchanger(
                (2, 9, 10), torch.float32, "cpu", width=w, nfields=nf,
                _force_remote=force)
            local = set(ex.local_directions)
            if force:
                assert not local
            seen = []
            for d, st, rf, n in ex.schedule():
                seen.append(d)
                assert st is not None or rf is not None
                h = w if d[0] else 9
                wd = w if d[1] else 10 - 2 * w
                assert n == nf * 2 * h * wd
                if d in local:
                    assert st == rank and rf == rank
                    continue
                if not force:
                    assert st != rank and rf != rank, \
                        "self must never be a remote peer"
                if st is not None:
                    sends.setdefault((rank, st), []).append(n)
                if rf is not None:
                    recvs.setdefault((rank, rf), []).append(n)
            # one message per direction, in the fixed global order
            order = [d for d in m.parallel.halo.DIRECTIONS if d in seen]
            assert seen == order and len(set(seen)) == len(seen)
        pairs = set(sends) | {(s, d) for (d, s) in recvs}
        for src, dst in pairs:
            assert sends.get((src, dst), []) == recvs.get((dst, src), []), \
                (dims, periodic, w, nf, src, dst)


# -------------------------------------------------------------- validation

def test_validation(grids):
    grid = grids[(True, True)]
    mk = grid.make_halo_exchanger
    with pytest.raises(ValueError, match="3\\*width"):
        mk((5, 9), torch.float32, "cpu", width=2)
    with pytest.raises(ValueError, match="3\\*width"):
        mk((9, 5), torch.float32, "cpu", width=2)
    with pytest.raises(ValueError, match="width"):
        mk((9, 9), torch.float32, "cpu", width=0)
    with pytest.raises(ValueError, match="nfields"):
        mk((9, 9), torch.float32, "cpu", nfields=0)
    with pytest.raises(ValueError, match="nfields"):
        mk((9, 9), torch.float32, "cpu", nfields=9)
    with pytest.raises(ValueError, match="2 dims"):
        mk((9,), torch.float32, "cpu")
    with pytest.raises(TypeError):
        mk((9, 9), "float32", "cpu")

    ex = mk((2, 9, 9), torch.float32, "cpu", width=2, nfields=2)
    a = torch.zeros(2, 9, 9)
    with pytest.raises(ValueError, match="2 field"):
        ex.exchange_(a)
    with pytest.raises(ValueError, match="2 field"):
        ex.exchange_(a, a, a)
    with pytest.raises(ValueError, match="shape"):
        ex.exchange_(a, torch.zeros(2, 9, 10))
    with pytest.raises(ValueError, match="shape"):
        ex.exchange_(a, torch.zeros(18, 9))
    with pytest.raises(TypeError, match="dtype"):
        ex.exchange_(a, a.double())
    with pytest.raises(ValueError, match="lives on"):
        ex.exchange_(a, a.to("meta"))
    with pytest.raises(ValueError, match="contiguous"):
        ex.exchange_(a, torch.zeros(2, 9, 18)[..., ::2])
    with pytest.raises(TypeError, match="Tensor"):
        ex.exchange_(a, 1.0)
    g = torch.zeros(2, 9, 9, requires_grad=True)
    with pytest.raises(ValueError,
                       match="not differentiable.*halo_exchange"):
        ex.exchange(a, g)
    # nothing was touched by the rejected calls
    assert torch.equal(a, torch.zeros(2, 9, 9))


def test_exported():
    from mpi4jax_amd import parallel

    assert parallel.HaloExchanger is parallel.halo.HaloExchanger


# ----------------------------------------------------------------- example

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = {k: v for k, v in os.environ.items()
       if not k.startswith(("RANK", "WORLD_SIZE", "MASTER_", "LOCAL_"))}
ENV["PYTHONPATH"] = REPO


@pytest.mark.parametrize("n", [1, 2])
def test_wide_stencil_example(n):
    cmd = [sys.executable, "examples/wide_stencil_diffusion.py",
           "--size", "32", "--nz", "3", "--steps", "5", "--device", "cpu"]
    if n > 1:
        cmd = [sys.executable, "-m", "mpi4jax_amd.run", "-n", str(n)] + cmd[1:]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300,
                         env=ENV, cwd=REPO)
    assert res.returncode == 0, res.stderr + res.stdout
    assert f"OK: 5 steps over {n} rank(s)" in res.stdout
