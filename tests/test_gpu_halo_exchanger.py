"""GPU suite for parallel/halo.HaloExchanger: the native executor
(csrc/halo.hip + bridge.cpp:halo_exchange_nd) at world 1.

Periodic self-wraps cover the local path (pack straight into the receive
staging buffer, no RCCL); ``_force_remote=True`` sends the same strips to
self through the RCCL group, the way tests/test_gpu_loopback.py drives
``sw_exchange``.  Every comparison is bitwise against the CPU exchanger
and the oracle of tests/test_halo_exchanger.py.
"""

import itertools

import pytest
import torch

import mpi4jax_amd as m
from mpi4jax_amd.parallel.grid import CartesianGrid
from test_halo_exchanger import world1_case

pytestmark = pytest.mark.gpu

OPEN = [(True, True), (False, True), (True, False)]
# one-cell interior, sizes off the 64/256 multiples, strips that cross a
# block boundary, batch dims
SHAPES = [(3, 3), (6, 6), (9, 9), (6, 131), (67, 6), (300, 7), (37, 53),
          (41, 70), (5, 11, 13), (2, 3, 9, 10)]


def _valid(shape, w):
    return shape[-2] >= 3 * w and shape[-1] >= 3 * w


@pytest.fixture(scope="module", autouse=True)
def _init():
    m.init()
    yield
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def grids():
    ps = OPEN + [(False, False)]
    return {p: CartesianGrid(dims=(1, 1), periodic=p) for p in ps}


def _ext():
    from mpi4jax_amd._backend import rccl

    return rccl.ext()


def _as_tuple(out):
    return out if isinstance(out, tuple) else (out,)


@pytest.mark.parametrize("periodic", OPEN)
@pytest.mark.parametrize("w", [1, 2, 3])
def test_local_path_matches_cpu_and_oracle(grids, periodic, w):
    grid = grids[periodic]
    dtypes = (torch.float32, torch.float64, torch.bfloat16, torch.uint8,
              torch.int64)
    ran = 0
    for shape, nf, dtype in itertools.product(SHAPES, (1, 3, 8), dtypes):
        if not _valid(shape, w):
            continue
        fields, exp = world1_case(shape, w, nf, dtype, periodic)
        cpu = _as_tuple(grid.make_halo_exchanger(
            shape, dtype, "cpu", width=w, nfields=nf).exchange(*fields))
        ex = grid.make_halo_exchanger(shape, dtype, "cuda", width=w,
                                      nfields=nf)
        dev = [f.cuda() for f in fields]
        got = _as_tuple(ex.exchange_(*dev))
        for g, c, e in zip(got, cpu, exp):
            g = g.cpu()
            assert torch.equal(g, c), (shape, nf, dtype)
            assert torch.equal(g, e), (shape, nf, dtype)
        ran += 1
    assert ran >= 3 * 5 * 5  # every width keeps at least five shapes


@pytest.mark.parametrize("periodic", OPEN)
@pytest.mark.parametrize("w", [1, 3])
def test_rccl_loopback_equals_local_path(grids, periodic, w):
    grid = grids[periodic]
    for shape, nf, dtype in itertools.product(
            SHAPES, (1, 3), (torch.float32, torch.uint8)):
        if not _valid(shape, w):
            continue
        fields, exp = world1_case(shape, w, nf, dtype, periodic, "cuda")
        local = _as_tuple(grid.make_halo_exchanger(
            shape, dtype, "cuda", width=w, nfields=nf).exchange(*fields))
        ex = grid.make_halo_exchanger(shape, dtype, "cuda", width=w,
                                      nfields=nf, _force_remote=True)
        assert not ex.local_directions
        remote = _as_tuple(ex.exchange(*fields))
        for r, lo, e in zip(remote, local, exp):
            assert torch.equal(r, lo), (shape, nf, dtype)
            assert torch.equal(r, e), (shape, nf, dtype)


def test_width1_2d_equals_halo_exchange(grids):
    torch.manual_seed(5)
    for periodic, grid in grids.items():
        for dtype in (torch.float32, torch.float64):
            a = torch.randn(37, 53, dtype=dtype, device="cuda")
            ex = grid.make_halo_exchanger(a.shape, dtype, "cuda")
            assert torch.equal(ex.exchange(a), grid.halo_exchange(a)), \
                (periodic, dtype)


def test_closed_grid_is_a_no_op_without_rccl(grids):
    """(F, F) at world 1 has no sender anywhere: the arrays stay as they
    are and no communicator is created."""
    grid = grids[(False, False)]
    before = _ext().comm_count()
    fields, _ = world1_case((2, 9, 10), 2, 3, torch.float32,
                            (False, False), "cuda")
    orig = [f.clone() for f in fields]
    ex = grid.make_halo_exchanger((2, 9, 10), torch.float32, "cuda",
                                  width=2, nfields=3)
    ex.exchange_(*fields)
    torch.cuda.synchronize()
    for f, x in zip(fields, orig):
        assert torch.equal(f, x)
    assert ex.schedule() == []
    assert _ext().comm_count() == before


def test_periodic_world1_needs_no_rccl(grids):
    before = _ext().comm_count()
    fields, exp = world1_case((37, 53), 2, 2, torch.float64, (True, True),
                              "cuda")
    ex = grids[(True, True)].make_halo_exchanger(
        (37, 53), torch.float64, "cuda", width=2, nfields=2)
    ex.exchange_(*fields)
    assert all(torch.equal(f, e) for f, e in zip(fields, exp))
    assert _ext().comm_count() == before


def test_python_executor_on_gpu_equals_native(grids, monkeypatch):
    for periodic, w in itertools.product(OPEN, (1, 2)):
        fields, exp = world1_case((5, 11, 13), w, 3, torch.float32,
                                  periodic, "cuda")
        ex = grids[periodic].make_halo_exchanger(
            (5, 11, 13), torch.float32, "cuda", width=w, nfields=3)
        monkeypatch.delenv("MPI4JAX_AMD_HALO_PY", raising=False)
        native = ex.exchange(*fields)
        monkeypatch.setenv("MPI4JAX_AMD_HALO_PY", "1")
        py = ex.exchange(*fields)
        for n, p, e in zip(native, py, exp):
            assert torch.equal(n, p)
            assert torch.equal(n, e)


def test_graph_capture_and_no_allocation(grids):
    shape, w, nf = (3, 41, 70), 2, 3
    grid = grids[(True, True)]
    ex = grid.make_halo_exchanger(shape, torch.float32, "cuda", width=w,
                                  nfields=nf)
    torch.manual_seed(9)
    fields = [torch.randn(shape, device="cuda") for _ in range(nf)]
    ex.exchange_(*fields)  # warm-up
    torch.cuda.synchronize()
    n0 = torch.cuda.memory_stats()["allocation.all.allocated"]
    ex.exchange_(*fields)
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == n0, \
        "exchange_ allocated after warm-up"

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ex.exchange_(*fields)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ex.exchange_(*fields)

    fresh = [torch.randn(shape, device="cuda") for _ in range(nf)]
    eager = grid.make_halo_exchanger(shape, torch.float32, "cuda", width=w,
                                     nfields=nf).exchange(*fresh)
    for f, x in zip(fields, fresh):
        f.copy_(x)
    graph.replay()
    torch.cuda.synchronize()
    for f, e, x in zip(fields, eager, fresh):
        assert torch.equal(f, e)
        assert not torch.equal(f, x)  # the replay did refresh the halos


@pytest.mark.parametrize("force_remote", [False, True])
def test_staging_poison(grids, force_remote):
    for dtype in (torch.float32, torch.uint8):
        fields, exp = world1_case((2, 9, 10), 2, 3, dtype, (True, True),
                                  "cuda")
        ex = grids[(True, True)].make_halo_exchanger(
            (2, 9, 10), dtype, "cuda", width=2, nfields=3,
            _force_remote=force_remote)
        ex._sbuf.view(torch.uint8).fill_(0xFF)  # NaN pattern for floats
        ex._rbuf.view(torch.uint8).fill_(0xFF)
        ex.exchange_(*fields)
        for f, e in zip(fields, exp):
            assert torch.equal(f, e)


def test_gpu_rejects_odd_element_size(grids):
    with pytest.raises(TypeError, match="1/2/4/8-byte"):
        grids[(True, True)].make_halo_exchanger(
            (9, 9), torch.complex128, "cuda")


def test_native_entry_validates(grids):
    """halo_exchange_nd checks every buffer and index itself."""
    ext = _ext()
    f = torch.zeros(2, 9, 10, device="cuda")
    buf = torch.zeros(4096, device="cuda")
    none = [-1] * 8
    wrap = [0, 0] + [-1] * 6
    ok = ([f], 2, 9, 10, 2, wrap, wrap, 0b11, buf, buf.clone(), -1)

    def call(**kw):
        names = ("fields", "levels", "ny", "nx", "width", "send_to",
                 "recv_from", "local_mask", "sbuf", "rbuf", "comm_id")
        args = dict(zip(names, ok))
        args.update(kw)
        ext.halo_exchange_nd(*(args[n] for n in names))

    call()
    for bad in (dict(fields=[]), dict(fields=[f] * 9), dict(width=0),
                dict(width=4), dict(ny=10), dict(levels=3),
                dict(send_to=none[:7]), dict(local_mask=256),
                dict(local_mask=0b100),  # local entry without peers
                dict(sbuf=buf[:8]), dict(rbuf=buf.double()),
                dict(sbuf=buf.cpu()), dict(fields=[f.cpu()]),
                dict(fields=[f.transpose(1, 2)]),
                dict(fields=[f, f.double()]),
                dict(send_to=[-2] + none[1:], local_mask=0),
                dict(fields=[torch.zeros(2, 9, 10, dtype=torch.complex128,
                                         device="cuda")])):
        with pytest.raises(RuntimeError):
            call(**bad)
    torch.cuda.synchronize()
    assert torch.equal(f, torch.zeros_like(f))


def test_offsets_past_2_31():
    """uint8 (1, 46400, 46400): 2.15e9 elements, so the north halo row and
    the high ends of both halo columns sit past 2^31."""
    ny = nx = 46400
    grid = CartesianGrid(dims=(1, 1), periodic=(True, True))
    f = torch.empty(1, ny, nx, dtype=torch.uint8, device="cuda")
    assert f.numel() > 1 << 31
    rows = (torch.arange(ny, device="cuda") * 7 % 256).to(torch.uint8)
    cols = (torch.arange(nx, device="cuda") * 13 % 256).to(torch.uint8)
    torch.add(rows[:, None], cols[None, :], out=f[0])  # wraps mod 256
    g = f[0]
    pre = dict(w=g[:, 1].clone(), e=g[:, nx - 2].clone(),
               s=g[1].clone(), n=g[ny - 2].clone(),
               inner=g[ny // 2, :].clone())
    ex = None
    try:
        ex = grid.make_halo_exchanger(f.shape, f.dtype, "cuda")
        ex.exchange_(f)
        # columns (full height minus the corners, which the diagonals own)
        assert torch.equal(g[1:-1, nx - 1], pre["w"][1:-1])
        assert torch.equal(g[1:-1, 0], pre["e"][1:-1])
        # rows over the interior columns
        assert torch.equal(g[0, 1:-1], pre["n"][1:-1])
        assert torch.equal(g[ny - 1, 1:-1], pre["s"][1:-1])
        # corners <- opposite interior corner cell
        assert g[ny - 1, nx - 1] == pre["s"][1]
        assert g[ny - 1, 0] == pre["s"][nx - 2]
        assert g[0, nx - 1] == pre["n"][1]
        assert g[0, 0] == pre["n"][nx - 2]
        # interior untouched
        assert torch.equal(g[ny // 2, 1:-1], pre["inner"][1:-1])
        assert torch.equal(g[1, 1:-1], pre["s"][1:-1])
    finally:
        del f, g, ex, pre
        torch.cuda.empty_cache()
