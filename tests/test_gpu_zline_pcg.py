"""GPU suite for the native line solve and the fused PCG update
(csrc/zline.hip + bridge.cpp:halo_zline_solve_nd / _pcg_update_nd) at world
1.  References, bounds and cases are those of tests/test_zline_pcg.py.
``_lds_planes`` in (0, 3, None): at nz = 7 the value 3 splits a column
between the LDS stash and the stash in ``z``.  The kernel's tile is 4 rows
x 64 columns, so (2, nz, 41, 70) spans 10 x 2 ragged tiles per column.
"""

import pytest
import torch

import mpi4jax_amd as m
from mpi4jax_amd.parallel.grid import CartesianGrid
from test_gpu_halo_exchanger import OPEN
from test_zline_pcg import (BANDS, F32_F64, SOLVE_CASES, ZB, dense_t,
                            run_anisotropic, run_solve, run_update,
                            test_diagonal_power_of_two_is_exact as exact,
                            weights)

pytestmark = pytest.mark.gpu

LDS = (0, 3, None)


@pytest.fixture(scope="module", autouse=True)
def _init():
    m.init()
    yield
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def grids():
    return {p: CartesianGrid(dims=(1, 1), periodic=p)
            for p in OPEN + [(False, False)]}


@pytest.mark.parametrize("lds", LDS)
@pytest.mark.parametrize("dtype", F32_F64)
@pytest.mark.parametrize("zb,nz", SOLVE_CASES)
def test_line_solve_matches_dense_and_cpu(grids, zb, nz, dtype, lds):
    worst, got = run_solve(grids, zb, nz, dtype, "cuda", lds)
    print("err / (eps kappa):", worst)
    _, cpu = run_solve(grids, zb, nz, dtype, "cpu")
    t = dense_t(nz, *BANDS, zb)
    kappa = (torch.linalg.matrix_norm(t, float("inf"))
             * torch.linalg.matrix_norm(torch.linalg.inv(t), float("inf")))
    for g, c in zip(got, cpu):
        assert ((g - c).abs().max() / c.abs().max()
                <= 16 * torch.finfo(dtype).eps * kappa)


@pytest.mark.parametrize("zb", ZB)
def test_diagonal_power_of_two_is_exact(grids, zb):
    exact(grids, zb, "cuda")


@pytest.mark.parametrize("lds", LDS)
@pytest.mark.parametrize("dtype", F32_F64)
@pytest.mark.parametrize("zb", ZB)
def test_update_matches_composition(grids, zb, dtype, lds):
    run_update(grids[(True, True)], zb, dtype, "cuda", lds)


def test_pcg_halves_the_iterations(grids):
    run_anisotropic(grids[(False, False)], "cuda")


def test_pcg_iteration_is_capturable(grids):
    """One replay of a graph of ``iterate(2)`` equals the eager result."""
    b = torch.nn.functional.pad(
        torch.randn(8, 12, 14, generator=torch.Generator().manual_seed(5)),
        (1, 1, 1, 1)).cuda()
    st = grids[(False, False)].make_stencil3d(
        b.shape, torch.float32, "cuda", weights(-100.0, 205.0, -100.0, -1.0),
        z_boundary="periodic")
    eager, cg = st.make_cg("zline"), st.make_cg("zline")
    x, xe = torch.zeros_like(b), torch.zeros_like(b)
    cg.start(b, x)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cg.iterate(2)  # warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cg.iterate(2)
    cg.start(b, x.zero_())  # the same x tensor the graph updates
    graph.replay()
    eager.start(b, xe)
    eager.iterate(2)
    torch.cuda.synchronize()
    assert torch.equal(x, xe) and x.any()
    assert torch.equal(cg.rz, eager.rz) and torch.equal(cg.rr, eager.rr)
