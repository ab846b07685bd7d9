"""GPU suite for the adjoint of parallel/halo.HaloExchanger: the native
executor (csrc/halo.hip: the adjoint pack mode of halo_nd_kernel and
halo_adjoint_acc_kernel; bridge.cpp:halo_adjoint_nd) at world 1.

Periodic self-wraps cover the local path; ``_force_remote=True`` sends the
same strips to self through the RCCL group.  Comparisons with the CPU
executor and the index-map oracle of tests/test_halo_adjoint.py use
integer data in [-4, 4] (every sum exact in every dtype); comparisons
between the native and the Python executor on the GPU use random normal
data, because both follow the same fixed order of adds.
"""

import itertools

import pytest
import torch

import mpi4jax_amd as m
from mpi4jax_amd.parallel.grid import CartesianGrid
from test_gpu_halo_exchanger import OPEN, SHAPES, _valid
from test_halo_adjoint import (DTYPES, int_data, oracle_adjoint,
                               source_map)

pytestmark = pytest.mark.gpu


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
    ran = 0
    for shape in SHAPES:
        if not _valid(shape, w):
            continue
        src = source_map(grid, shape, w)
        for nf, dtype in itertools.product((1, 3, 8), DTYPES):
            gout = [int_data(shape, dtype, 31 * k + nf) for k in range(nf)]
            cpu = _as_tuple(grid.make_halo_exchanger(
                shape, dtype, "cpu", width=w, nfields=nf).adjoint(*gout))
            ex = grid.make_halo_exchanger(shape, dtype, "cuda", width=w,
                                          nfields=nf)
            got = _as_tuple(ex.adjoint_(*[g.cuda() for g in gout]))
            for g, c, o in zip(got, cpu, gout):
                g = g.cpu()
                assert torch.equal(g, c), (shape, nf, dtype)
                assert torch.equal(g.double(), oracle_adjoint(src, o)), \
                    (shape, nf, dtype)
            ran += 1
    assert ran >= 5 * 3 * 4  # every width keeps at least five shapes


@pytest.mark.parametrize("periodic", OPEN)
@pytest.mark.parametrize("w", [1, 3])
def test_rccl_loopback_equals_local_path(grids, periodic, w):
    grid = grids[periodic]
    for shape, nf, dtype in itertools.product(
            SHAPES, (1, 3), (torch.float32, torch.bfloat16)):
        if not _valid(shape, w):
            continue
        gout = [int_data(shape, dtype, 7 * k + nf, "cuda")
                for k in range(nf)]
        local = _as_tuple(grid.make_halo_exchanger(
            shape, dtype, "cuda", width=w, nfields=nf).adjoint(*gout))
        ex = grid.make_halo_exchanger(shape, dtype, "cuda", width=w,
                                      nfields=nf, _force_remote=True)
        assert not ex.local_directions
        remote = _as_tuple(ex.adjoint(*gout))
        for r, lo in zip(remote, local):
            assert torch.equal(r, lo), (shape, nf, dtype)


def test_native_equals_python_executor_on_random_data(grids, monkeypatch):
    """Random normal data: equal only if both add in the same order."""
    torch.manual_seed(21)
    cases = [((3, 3), 1), ((6, 6), 2), ((9, 9), 3), ((5, 11, 13), 2),
             ((37, 53), 1), ((2, 3, 9, 10), 3)]
    for periodic, (shape, w), dtype in itertools.product(
            OPEN, cases, (torch.float32, torch.float64)):
        ex = grids[periodic].make_halo_exchanger(
            shape, dtype, "cuda", width=w, nfields=3)
        gout = [torch.randn(shape, dtype=dtype, device="cuda")
                for _ in range(3)]
        monkeypatch.delenv("MPI4JAX_AMD_HALO_PY", raising=False)
        native = ex.adjoint(*gout)
        monkeypatch.setenv("MPI4JAX_AMD_HALO_PY", "1")
        py = ex.adjoint(*gout)
        monkeypatch.delenv("MPI4JAX_AMD_HALO_PY")
        for n, p in zip(native, py):
            assert torch.equal(n, p), (periodic, shape, w, dtype)


def test_closed_grid_is_a_no_op_without_rccl(grids):
    before = _ext().comm_count()
    gout = [torch.randn(2, 9, 10, device="cuda") for _ in range(3)]
    orig = [g.clone() for g in gout]
    ex = grids[(False, False)].make_halo_exchanger(
        (2, 9, 10), torch.float32, "cuda", width=2, nfields=3)
    ex.adjoint_(*gout)
    torch.cuda.synchronize()
    for g, x in zip(gout, orig):
        assert torch.equal(g, x)
    assert ex.adjoint_schedule() == []
    assert _ext().comm_count() == before


def test_periodic_world1_needs_no_rccl(grids):
    before = _ext().comm_count()
    shape = (37, 53)
    src = source_map(grids[(True, True)], shape, 2)
    gout = [int_data(shape, torch.float64, k, "cuda") for k in range(2)]
    orig = [g.clone() for g in gout]
    ex = grids[(True, True)].make_halo_exchanger(
        shape, torch.float64, "cuda", width=2, nfields=2)
    ex.adjoint_(*gout)
    for g, o in zip(gout, orig):
        assert torch.equal(g.cpu(), oracle_adjoint(src, o))
    assert _ext().comm_count() == before


def test_exchange_ad_backward_matches_cpu(grids):
    shape, w = (5, 11, 13), 2
    for periodic in OPEN:
        grads = {}
        for device in ("cpu", "cuda"):
            ex = grids[periodic].make_halo_exchanger(
                shape, torch.float32, device, width=w, nfields=2)
            a = int_data(shape, torch.float32, 1, device).requires_grad_()
            b = int_data(shape, torch.float32, 2, device).requires_grad_()
            oa, ob = ex.exchange_ad(a, b)
            ref = ex.exchange(a.detach(), b.detach())
            assert torch.equal(oa.detach(), ref[0])
            assert torch.equal(ob.detach(), ref[1])
            wa = int_data(shape, torch.float32, 3, device)
            wb = int_data(shape, torch.float32, 4, device)
            ((oa * wa).sum() + (ob * wb).sum()).backward()
            grads[device] = (a.grad.cpu(), b.grad.cpu())
        for c, g in zip(grads["cpu"], grads["cuda"]):
            assert torch.equal(c, g), periodic


def test_gradcheck_on_gpu(grids):
    torch.manual_seed(22)
    ex = grids[(True, True)].make_halo_exchanger(
        (2, 6, 7), torch.float64, "cuda", width=2, nfields=2)
    a = torch.randn(2, 6, 7, dtype=torch.float64, device="cuda",
                    requires_grad=True)
    b = torch.randn(2, 6, 7, dtype=torch.float64, device="cuda")
    assert torch.autograd.gradcheck(lambda x: ex.exchange_ad(x, b), (a,))


def test_graph_capture_and_no_allocation(grids):
    shape, w, nf = (3, 41, 70), 2, 3
    grid = grids[(True, True)]
    ex = grid.make_halo_exchanger(shape, torch.float32, "cuda", width=w,
                                  nfields=nf)
    torch.manual_seed(9)
    gout = [torch.randn(shape, device="cuda") for _ in range(nf)]
    ex.adjoint_(*gout)  # warm-up
    torch.cuda.synchronize()
    n0 = torch.cuda.memory_stats()["allocation.all.allocated"]
    ex.adjoint_(*gout)
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == n0, \
        "adjoint_ allocated after warm-up"

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ex.adjoint_(*gout)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ex.adjoint_(*gout)

    fresh = [torch.randn(shape, device="cuda") for _ in range(nf)]
    eager = grid.make_halo_exchanger(shape, torch.float32, "cuda", width=w,
                                     nfields=nf).adjoint(*fresh)
    for g, x in zip(gout, fresh):
        g.copy_(x)
    graph.replay()
    torch.cuda.synchronize()
    for g, e, x in zip(gout, eager, fresh):
        assert torch.equal(g, e)
        assert not torch.equal(g, x)  # the replay did run the adjoint


@pytest.mark.parametrize("force_remote", [False, True])
def test_staging_poison(grids, force_remote):
    """NaN-filled staging: a forgotten zero store for the skipped corner
    rows of a column slot, or an accumulate from a slot no one filled,
    would show."""
    shape, w, nf = (2, 9, 10), 2, 3
    for periodic, dtype in itertools.product(
            OPEN, (torch.float32, torch.bfloat16)):
        src = source_map(grids[periodic], shape, w)
        gout = [int_data(shape, dtype, k, "cuda") for k in range(nf)]
        orig = [g.clone() for g in gout]
        ex = grids[periodic].make_halo_exchanger(
            shape, dtype, "cuda", width=w, nfields=nf,
            _force_remote=force_remote)
        ex._sbuf.view(torch.uint8).fill_(0xFF)  # NaN pattern
        ex._rbuf.view(torch.uint8).fill_(0xFF)
        ex.adjoint_(*gout)
        for g, o in zip(gout, orig):
            assert torch.equal(g.cpu().double(), oracle_adjoint(src, o))


def test_native_entry_validates(grids):
    """halo_adjoint_nd checks every buffer and index itself."""
    ext = _ext()
    f = torch.zeros(2, 9, 10, device="cuda")
    buf = torch.zeros(4096, device="cuda")
    none = [-1] * 8
    wrap = [0, 0] + [-1] * 6
    ok = ([f], 2, 9, 10, 2, wrap, wrap, 0b11, buf, buf.clone(), -1)
    names = ("fields", "levels", "ny", "nx", "width", "send_to",
             "recv_from", "local_mask", "sbuf", "rbuf", "comm_id")

    def call(**kw):
        args = dict(zip(names, ok))
        args.update(kw)
        ext.halo_adjoint_nd(*(args[n] for n in names))

    call()
    fi = torch.zeros(2, 9, 10, dtype=torch.int32, device="cuda")
    bi = torch.zeros(4096, dtype=torch.int32, device="cuda")
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
                                         device="cuda")]),
                # the adjoint is arithmetic: floating dtypes only
                dict(fields=[fi], sbuf=bi, rbuf=bi.clone()),
                dict(sbuf=bi, rbuf=bi.clone())):
        with pytest.raises((RuntimeError, ValueError)):
            call(**bad)
    torch.cuda.synchronize()
    assert torch.equal(f, torch.zeros_like(f))
    assert torch.equal(fi, torch.zeros_like(fi))


def test_work_items_past_2_31_are_rejected(grids):
    """(1, n, 3) at width 1 is all frame; eight such float16 fields pass
    2^31 work items while the staging (two thirds of that) still fits.
    Building the exchanger works — the forward exchange has no such limit
    — and the adjoint refuses at call time, in Python and in the entry."""
    n = 89_500_000
    assert 8 * 3 * n >= 1 << 31
    f = ex = None
    try:
        f = torch.zeros(1, n, 3, dtype=torch.float16, device="cuda")
        ex = grids[(True, True)].make_halo_exchanger(
            f.shape, f.dtype, "cuda", nfields=8)
        with pytest.raises(ValueError, match="2\\^31"):
            ex.adjoint_(*[f] * 8)
        with pytest.raises(ValueError, match="2\\^31"):
            _ext().halo_adjoint_nd(
                [f] * 8, 1, n, 3, 1, ex._send_to, ex._recv_from,
                ex._local_mask, ex._sbuf, ex._rbuf, -1)
        torch.cuda.synchronize()
        assert int(torch.count_nonzero(f)) == 0
    finally:
        del f, ex
        torch.cuda.empty_cache()


def test_offsets_past_2_31():
    """float16 (1, 46400, 46400): 2.15e9 elements, so the north rows and
    the high ends of the side bands sit past 2^31.  Width 1, periodic:
    halo cells are zeroed, the interior ring collects its own value plus
    the opposite halo's, and an interior corner cell collects four."""
    ny = nx = 46400
    grid = CartesianGrid(dims=(1, 1), periodic=(True, True))
    f = g = ex = pre = None
    try:
        f = torch.zeros(1, ny, nx, dtype=torch.float16, device="cuda")
        assert f.numel() > 1 << 31
        g = f[0]
        ramp = torch.arange(nx, device="cuda")
        for k, j in enumerate((0, 1, ny - 2, ny - 1)):
            g[j] = ((ramp * (k + 2)) % 7 - 3).to(torch.float16)
            g[:, j] = ((ramp * (k + 3)) % 5 - 2).to(torch.float16)
        pre = dict(r0=g[0].clone(), r1=g[1].clone(), rm=g[ny - 2].clone(),
                   rn=g[ny - 1].clone(), c0=g[:, 0].clone(),
                   c1=g[:, 1].clone(), cm=g[:, nx - 2].clone(),
                   cn=g[:, nx - 1].clone(), inner=g[ny // 2].clone())
        ex = grid.make_halo_exchanger(f.shape, f.dtype, "cuda")
        ex.adjoint_(f)
        # the halo ring was overwritten in the forward pass
        for halo in (g[0], g[ny - 1], g[:, 0], g[:, nx - 1]):
            assert int(torch.count_nonzero(halo)) == 0
        # west / east interior columns, away from the corner cells
        assert torch.equal(g[2:-2, 1], pre["c1"][2:-2] + pre["cn"][2:-2])
        assert torch.equal(g[2:-2, nx - 2],
                           pre["cm"][2:-2] + pre["c0"][2:-2])
        # south / north interior rows
        assert torch.equal(g[1, 2:-2], pre["r1"][2:-2] + pre["rn"][2:-2])
        assert torch.equal(g[ny - 2, 2:-2],
                           pre["rm"][2:-2] + pre["r0"][2:-2])
        # interior corner cells: own + diagonal + row + column terms
        assert g[1, 1] == (pre["r1"][1] + pre["rn"][nx - 1] + pre["rn"][1]
                           + pre["r1"][nx - 1])
        assert g[1, nx - 2] == (pre["r1"][nx - 2] + pre["rn"][0]
                                + pre["rn"][nx - 2] + pre["r1"][0])
        assert g[ny - 2, 1] == (pre["rm"][1] + pre["r0"][nx - 1]
                                + pre["r0"][1] + pre["rm"][nx - 1])
        assert g[ny - 2, nx - 2] == (pre["rm"][nx - 2] + pre["r0"][0]
                                     + pre["r0"][nx - 2] + pre["rm"][0])
        # a mid-field row is untouched off the two side bands
        assert torch.equal(g[ny // 2, 2:-2], pre["inner"][2:-2])
        assert int(torch.count_nonzero(g[ny // 2, 2:-2])) == 0
    finally:
        del f, g, ex, pre
        torch.cuda.empty_cache()
