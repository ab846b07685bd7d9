"""GPU suite for parallel/stencil3d.HaloStencil3D: the native executor
(csrc/stencil3d.hip + bridge.cpp:halo_stencil3d_nd / _dot_nd /
_adjoint_nd) at world 1.  Oracle, data and tap sets are those of
tests/test_stencil3d.py.  ``_z_chunk`` in (1, 3, nz) gives, at nz = 7,
chunks of 3, 3, 1: a ragged last chunk and chunks shorter than the reach
``2 rz``.
"""

import itertools

import pytest
import torch
import torch.nn.functional as F

import mpi4jax_amd as m
from mpi4jax_amd.parallel.grid import CartesianGrid
from test_gpu_halo_exchanger import OPEN
from test_gpu_halo_stencil import check_executors_agree
from test_halo_adjoint import int_data
from test_halo_stencil import as_tuple, check_bound, interior
from test_stencil_cg import int_dot
from test_stencil3d import (DTYPES, LAP7, SOLVES, TAPSETS, ZB, cg_cap,
                            check_cg, oracle)

pytestmark = pytest.mark.gpu

ALL = OPEN + [(False, False)]


@pytest.fixture(scope="module", autouse=True)
def _init():
    m.init()
    yield
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def grids():
    return {p: CartesianGrid(dims=(1, 1), periodic=p) for p in ALL}


def shapes_for(k, zb):
    """One plane (zero boundary only), every plane at both z ends, the
    periodic minimum, two ragged multi-tile columns with nz = 7, and a
    fast-fill tile at every width."""
    rz, w = (k.shape[0] - 1) // 2, (k.shape[1] - 1) // 2
    small = [(nz, 3 * w, 3 * w + 1) for nz in sorted({1, max(rz, 1)})
             if nz >= (2 * rz + 1 if zb == "periodic" else 1)]
    return small + [(2 * rz + 1, max(9, 3 * w), 14), (2, 7, 41, 70),
                    (5, 76, 140)]


def run_exact(grid, k, zb, shape, nf, dtypes, **kw):
    """apply, apply_dot and adjoint on integer data: bitwise against the
    float64 oracle and the CPU executor, ``<A x, y> == <x, A^T y>`` and
    ``pAp`` exact in int64, inputs unmutated, ``gin`` finite."""
    w, nz = (k.shape[1] - 1) // 2, shape[-3]
    base = [int_data(shape, torch.float64, 7 * i + nf) for i in range(nf)]
    exp = oracle(grid, k, base, zb)
    for dtype in dtypes:
        x = [f.to(dtype) for f in base]
        y = [int_data(shape, dtype, 50 + i) for i in range(nf)]
        cpu = grid.make_stencil3d(shape, dtype, "cpu", k, nfields=nf,
                                  z_boundary=zb)
        cpu_out, cpu_gin = as_tuple(cpu.apply(*x)), as_tuple(cpu.adjoint(*y))
        dx, dy = [f.cuda() for f in x], [f.cuda() for f in y]
        for zc in sorted({min(c, nz) for c in (1, 3, nz)}):
            what = (shape, nf, dtype, zc)
            st = grid.make_stencil3d(shape, dtype, "cuda", k, nfields=nf,
                                     z_boundary=zb, _z_chunk=zc, **kw)
            assert st.z_chunk == zc
            got = as_tuple(st.apply(*dx))
            gin = as_tuple(st.adjoint(*dy))
            out, pap = st.apply_dot(*dx)
            _, pap2 = st.apply_dot(*dx)
            for g, c, e, o in zip(got, cpu_out, exp, as_tuple(out)):
                assert torch.equal(g.cpu(), c), what
                assert torch.equal(interior(g.cpu(), w).double(), e), what
                assert torch.equal(o, g), what
            for g, c in zip(gin, cpu_gin):
                assert torch.isfinite(g).all() and torch.equal(g.cpu(), c), \
                    what
            for d, f in zip(dx + dy, x + y):
                assert torch.equal(d.cpu(), f), "an input was mutated"
            if dtype in (torch.float32, torch.float64):
                ax_y = sum(int_dot(a, b) for a, b in zip(got, y))
                assert ax_y == sum(int_dot(a, b) for a, b in zip(x, gin)), \
                    what
            assert pap.item() == sum(int_dot(a, b)
                                     for a, b in zip(x, got)), what
            assert torch.equal(pap, pap2), what


@pytest.mark.parametrize("periodic", ALL)
@pytest.mark.parametrize("zb", ZB)
@pytest.mark.parametrize("name", list(TAPSETS))
def test_exact(grids, name, zb, periodic):
    k = TAPSETS[name]
    for shape, nf in itertools.product(shapes_for(k, zb), (1, 3)):
        run_exact(grids[periodic], k, zb, shape, nf, DTYPES)


@pytest.mark.parametrize("periodic", OPEN)
@pytest.mark.parametrize("zb", ZB)
@pytest.mark.parametrize("name", ["star7", "box27"])
def test_staged_exact(grids, name, zb, periodic):
    k = TAPSETS[name]
    for shape, nf in itertools.product(shapes_for(k, zb)[:3], (1, 3)):
        run_exact(grids[periodic], k, zb, shape, nf,
                  (torch.float32, torch.bfloat16), _force_remote=True)


@pytest.mark.parametrize("force_remote", [False, True])
@pytest.mark.parametrize("zb", ZB)
def test_executors_agree_on_ragged_tiles(grids, zb, force_remote,
                                         monkeypatch):
    """A ragged tile edge in both directions and a ragged last chunk of
    planes (nz = 3 in chunks of 2), two columns, both launch sequences:
    every native entry of the family against the Python executor."""
    shape = (2, 3, 35, 67)
    for dtype in (torch.float32, torch.float64):  # every value is exact
        st = grids[(True, True)].make_stencil3d(
            shape, dtype, "cuda", TAPSETS["box27"], nfields=2,
            z_boundary=zb, _z_chunk=2, _force_remote=force_remote)
        x = [int_data(shape, dtype, i, "cuda") for i in range(2)]
        check_executors_agree(st, x, monkeypatch)


def test_adjoint_checks_the_communicator_before_its_launch(grids):
    """halo_stencil3d_adjoint_nd with a remote entry and a communicator
    that does not exist raises and leaves the sentinel-filled outputs
    alone: the lookup comes before the transposed launch."""
    from mpi4jax_amd._backend import rccl

    shape = (2, 3, 35, 67)
    st = grids[(True, True)].make_stencil3d(
        shape, torch.float32, "cuda", TAPSETS["star7"], _z_chunk=2,
        _force_remote=True)
    g = int_data(shape, torch.float32, 3, "cuda")
    out = torch.full(shape, 7.0, device="cuda")
    ex = st.exchanger
    with pytest.raises(RuntimeError, match="unknown RCCL communicator"):
        rccl.ext().halo_stencil3d_adjoint_nd(
            *st._native_args([g], [out]), ex._send_to, ex._recv_from,
            ex._local_mask, ex._sbuf, ex._rbuf, 123456)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


@pytest.mark.parametrize("zb", ZB)
@pytest.mark.parametrize("dtype", DTYPES)
def test_rounding_within_bound(grids, dtype, zb):
    torch.manual_seed(17)
    shape = (5, 76, 140)
    k = torch.randn(3, 3, 3, dtype=torch.float64)
    for periodic in ALL:
        x = [torch.randn(shape).to(dtype)]
        st = grids[periodic].make_stencil3d(shape, dtype, "cuda", k,
                                            z_boundary=zb)
        (e,), (g,) = oracle(grids[periodic], k, x, zb, with_mag=True)
        check_bound(interior(st.apply(x[0].cuda()), 1), e, g, 27, dtype,
                    periodic)


@pytest.mark.parametrize("dtype,rtol", SOLVES)
def test_cg_solves_3d(grids, dtype, rtol):
    grid = grids[(False, False)]
    *_, its = check_cg(grid, dtype, rtol, cg_cap(rtol))
    st, b, x, _ = check_cg(grid, dtype, rtol, its + 2, "cuda")
    x2, _ = st.make_cg().solve(b, rtol=rtol, maxiter=its + 2, check_every=1)
    assert torch.equal(x, x2), "two solves differ"


def test_cg_iteration_is_capturable(grids):
    """StencilCG.iterate with the 3-D kernel allocates nothing, so a graph
    of it replays to the eager result (several replays)."""
    b = F.pad(torch.randn(4, 10, 12,
                          generator=torch.Generator().manual_seed(5)),
              (1, 1, 1, 1)).cuda()
    st = grids[(True, False)].make_stencil3d(b.shape, torch.float32, "cuda",
                                             LAP7)
    eager, cg = st.make_cg(), st.make_cg()
    x, xe = torch.zeros_like(b), torch.zeros_like(b)
    cg.start(b, x)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cg.iterate(1)  # warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cg.iterate(1)
    cg.start(b, x.zero_())  # the same x tensor the graph updates
    for _ in range(3):
        graph.replay()
    eager.start(b, xe)
    eager.iterate(3)
    torch.cuda.synchronize()
    assert torch.equal(x, xe) and x.any()
