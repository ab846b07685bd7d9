"""GPU suite for parallel/varstencil.VariableHaloStencil: the native
executor (csrc/varstencil.hip + bridge.cpp:halo_varstencil_nd / _dot_nd /
_adjoint_nd) at world 1.  Oracle, data and tap sets are those of
tests/test_variable_stencil.py; ``_levels_per_block`` in (1, 2, 5) gives a
block one level, a march with a ragged last chunk, and the full march.
"""

import itertools

import pytest
import torch

import mpi4jax_amd as m
from mpi4jax_amd.parallel.grid import CartesianGrid
from test_gpu_halo_exchanger import OPEN
from test_gpu_halo_stencil import check_executors_agree
from test_halo_adjoint import int_data
from test_halo_stencil import as_tuple, check_bound, interior
from test_stencil_cg import int_dot
from test_variable_stencil import (DTYPES, SOLVES, TAPSETS, check_cg,
                                   int_coef, nan_halo, oracle, radius,
                                   shapes_for)

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


def lpbs(shape, choices):
    levels = shape[0] if len(shape) == 3 else 1
    return sorted({min(c, levels) for c in choices})


def run_exact(grid, offsets, shape, nf, lpb_choices, dtypes, **kw):
    """apply, apply_dot and adjoint on integer data: bitwise against the
    float64 oracle and the CPU executor, ``<A x, y> == <x, A^T y>`` and
    ``pAp`` exact in int64, inputs unmutated, ``gin`` finite."""
    w = radius(offsets)
    coef = int_coef(offsets, shape, nf)
    base = [int_data(shape, torch.float64, 7 * i + nf) for i in range(nf)]
    exp = oracle(grid, offsets, coef, base)
    for dtype in dtypes:
        x = [f.to(dtype) for f in base]
        y = [int_data(shape, dtype, 50 + i) for i in range(nf)]
        cpu = grid.make_variable_stencil(shape, dtype, "cpu", offsets, coef,
                                         nfields=nf)
        cpu_out, cpu_gin = as_tuple(cpu.apply(*x)), as_tuple(cpu.adjoint(*y))
        dx, dy = [f.cuda() for f in x], [f.cuda() for f in y]
        for lpb in lpbs(shape, lpb_choices):
            what = (shape, nf, dtype, lpb)
            st = grid.make_variable_stencil(
                shape, dtype, "cuda", offsets, coef, nfields=nf,
                _levels_per_block=lpb, **kw)
            assert st.levels_per_block == lpb
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
@pytest.mark.parametrize("name", list(TAPSETS))
def test_direct_path_exact(grids, periodic, name):
    offsets = TAPSETS[name]
    for shape, nf in itertools.product(shapes_for(radius(offsets)), (1, 3)):
        run_exact(grids[periodic], offsets, shape, nf, (1, 2, 5), DTYPES)


@pytest.mark.parametrize("periodic", OPEN)
@pytest.mark.parametrize("name", ["star5", "asym4"])
def test_staged_path_exact(grids, periodic, name):
    offsets = TAPSETS[name]
    for shape in shapes_for(radius(offsets))[:2]:
        run_exact(grids[periodic], offsets, shape, 3, (1, 2),
                  (torch.float32, torch.bfloat16), _force_remote=True)


@pytest.mark.parametrize("force_remote", [False, True])
def test_executors_agree_on_ragged_tiles(grids, force_remote, monkeypatch):
    """A ragged tile edge in both directions and a ragged last chunk of
    levels, both launch sequences: every native entry of the family against
    the Python executor."""
    offsets, shape = TAPSETS["box9"], (3, 35, 67)
    for dtype in (torch.float32, torch.float64):  # every value is exact
        st = grids[(True, True)].make_variable_stencil(
            shape, dtype, "cuda", offsets, int_coef(offsets, shape, 2),
            nfields=2, _levels_per_block=2, _force_remote=force_remote)
        x = [int_data(shape, dtype, i, "cuda") for i in range(2)]
        check_executors_agree(st, x, monkeypatch)


def test_adjoint_checks_the_communicator_before_its_launch(grids):
    """halo_varstencil_adjoint_nd with a remote entry and a communicator
    that does not exist raises and leaves the sentinel-filled outputs
    alone: the lookup comes before the transposed launch."""
    from mpi4jax_amd._backend import rccl

    offsets, shape = TAPSETS["star5"], (3, 35, 67)
    st = grids[(True, True)].make_variable_stencil(
        shape, torch.float32, "cuda", offsets, int_coef(offsets, shape, 1),
        _levels_per_block=2, _force_remote=True)
    g = int_data(shape, torch.float32, 3, "cuda")
    out = torch.full(shape, 7.0, device="cuda")
    ex = st.exchanger
    with pytest.raises(RuntimeError, match="unknown RCCL communicator"):
        rccl.ext().halo_varstencil_adjoint_nd(
            *st._native_args([g], [out]), ex._send_to, ex._recv_from,
            ex._local_mask, ex._sbuf, ex._rbuf, 123456)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_rounding_within_bound(grids, dtype):
    torch.manual_seed(17)
    offsets, shape = TAPSETS["box9"], (2, 76, 140)
    coef = nan_halo(torch.randn(9, 76, 140, dtype=torch.float64), 1)
    for periodic in ALL:
        x = [torch.randn(shape).to(dtype)]
        st = grids[periodic].make_variable_stencil(shape, dtype, "cuda",
                                                   offsets, coef)
        (e,), (g,) = oracle(grids[periodic], offsets, coef, x, with_mag=True)
        check_bound(interior(st.apply(x[0].cuda()), 1), e, g, 9, dtype,
                    periodic)


@pytest.mark.parametrize("periodic", [(True, False), (False, False)])
def test_cg_solves_variable_diffusion(grids, periodic):
    for dtype, rtol, cap in SOLVES:
        st, b, x = check_cg(grids[periodic], dtype, rtol, cap, "cuda")
        x2, _ = st.make_cg().solve(b, rtol=rtol, maxiter=cap, check_every=1)
        assert torch.equal(x, x2), "two solves differ"


def test_cg_iteration_is_capturable(grids):
    """StencilCG.iterate with the variable kernel allocates nothing, so a
    graph of it replays to the eager result (several replays)."""
    from test_variable_stencil import diffusion_system

    st, _, b = diffusion_system(grids[(True, False)], torch.float32, "cuda")
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
