"""CPU suite for parallel/zline.ZLineSolver and parallel/pcg.StencilPCG, and
the checks it shares with tests/test_gpu_zline_pcg.py.

Reference of a line solve: the dense float64 ``T`` and
``torch.linalg.solve`` along z.  Bound: ``|z - z_ref|_inf / |z_ref|_inf <=
16 eps kappa_inf(T)``.  LU of a diagonally dominant tridiagonal has
``|L||U| <= 3 |T|`` and the solve ``f(u) ~ 4u``, which gives ``6 eps
kappa``; the rest is margin for the rounded reciprocal tables.  The bands
``(-1.5, 3, -1)`` are diagonally dominant and not symmetric, so a swap of
``a`` and ``c`` shows.
"""

import pytest
import torch

import mpi4jax_amd as m
from mpi4jax_amd.parallel import StencilCG, StencilPCG, ZLineSolver
from mpi4jax_amd.parallel.grid import CartesianGrid
from test_halo_adjoint import int_data
from test_halo_exchanger import PERIODIC
from test_halo_stencil import as_tuple, interior
from test_stencil_cg import int_dot
from test_stencil3d import ZB, oracle

F32_F64 = (torch.float32, torch.float64)
BANDS = (-1.5, 3.0, -1.0)
NZS = {"zero": (1, 2, 3, 7), "periodic": (3, 7)}
SOLVE_CASES = [(zb, nz) for zb in ZB for nz in NZS[zb]]


def weights(a, b, c, h=-0.25):
    """Bands ``(a, b, c)`` along z and ``h`` on the four in-plane
    neighbours."""
    k = torch.zeros(3, 3, 3, dtype=torch.float64)
    k[0, 1, 1], k[1, 1, 1], k[2, 1, 1] = a, b, c
    k[1, 0, 1] = k[1, 2, 1] = k[1, 1, 0] = k[1, 1, 2] = h
    return k


def dense_t(nz, a, b, c, zb):
    t = (torch.diag(torch.full((nz,), b, dtype=torch.float64))
         + torch.diag(torch.full((nz - 1,), a, dtype=torch.float64), -1)
         + torch.diag(torch.full((nz - 1,), c, dtype=torch.float64), 1))
    if zb == "periodic":
        t[0, nz - 1] += a
        t[nz - 1, 0] += c
    return t


def check_solution(z, r, t, dtype, what):
    """``z`` against ``T^{-1} r`` on the interior (w = 1), its halo zero;
    returns the error over ``eps kappa``."""
    nz = t.shape[0]
    ri = interior(r.cpu().double(), 1)
    ref = torch.linalg.solve(
        t, ri.reshape(-1, nz, ri.shape[-2] * ri.shape[-1]))
    got = interior(z.cpu().double(), 1).reshape(ref.shape)
    kappa = (torch.linalg.matrix_norm(t, float("inf"))
             * torch.linalg.matrix_norm(torch.linalg.inv(t), float("inf")))
    ratio = ((got - ref).abs().max() / ref.abs().max()
             / (torch.finfo(dtype).eps * kappa)).item()
    assert ratio <= 16.0, (what, ratio)
    halo = z.clone()
    interior(halo, 1).zero_()
    assert not halo.any(), (what, "halo written")
    return ratio


def run_solve(grids, zb, nz, dtype, device, lds=None):
    """``solve`` at the tiny shape on every grid and at the ragged batched
    shape, one and two fields; returns the largest ratio and the outputs."""
    t = dense_t(nz, *BANDS, zb)
    worst, outs = 0.0, []
    cases = [(p, (nz, 3, 4)) for p in grids] + [((True, True),
                                                 (2, nz, 41, 70))]
    for (periodic, shape), nf in [(c, nf) for c in cases for nf in (1, 2)]:
        st = grids[periodic].make_stencil3d(
            shape, dtype, device, weights(*BANDS), nfields=nf, z_boundary=zb)
        ls = st.make_line_solver(_lds_planes=lds and min(lds, nz))
        assert isinstance(ls, ZLineSolver) and ls.bands == BANDS
        g = torch.Generator().manual_seed(nz + nf)
        r = [torch.randn(shape, generator=g, dtype=torch.float64).to(dtype)
             .to(device) for _ in range(nf)]
        keep = [f.clone() for f in r]
        z = as_tuple(ls.solve(*r))
        for fz, fr, fk in zip(z, r, keep):
            assert torch.equal(fr, fk), "solve() mutated its input"
            worst = max(worst, check_solution(
                fz, fr, t, dtype, (zb, shape, nf, dtype, lds)))
        outs += [f.cpu() for f in z]
    return worst, outs


def run_update(grid, zb, dtype, device, lds=None):
    """One fused update against ``StencilCG.update_step`` and the dense
    solve, on integer data with ``alpha = 2``."""
    shape, nf, w = (2, 7, 41, 70), 2, 1
    st = grid.make_stencil3d(shape, dtype, device, weights(*BANDS),
                             nfields=nf, z_boundary=zb)
    cg, pcg, again = st.make_cg(), st.make_cg("zline", _lds_planes=lds), \
        st.make_cg("zline", _lds_planes=lds)
    assert type(cg) is StencilCG and isinstance(pcg, StencilPCG)

    def load(s, pq):
        for name, seed in (("_x", 1), ("_r", 2), ("_p", 3), ("_q", 4)):
            setattr(s, name, [int_data(shape, dtype, seed + 10 * i, device)
                              for i in range(nf)])
        s._rs.fill_(4.0), s._pq.fill_(pq)

    for s in (cg, pcg, again):
        load(s, 2.0)
        s.update_step()
    for a, b in zip(cg._x + cg._r, pcg._x + pcg._r):
        assert torch.equal(interior(a, w), interior(b, w))
    assert pcg.rr.item() == sum(int_dot(interior(f, w), interior(f, w))
                                for f in pcg._r)
    assert pcg.rz_old.item() == 4.0
    t = dense_t(7, *BANDS, zb)
    zs = as_tuple(pcg.preconditioned_residual)
    for fz, fr in zip(zs, pcg._r):
        check_solution(fz, fr, t, dtype, (zb, dtype, lds))
    assert pcg.rz.item() == pytest.approx(st.dot(pcg._r, zs).item(),
                                          rel=1e-12)
    for a, b in zip(zs + (pcg.rz,), as_tuple(again.preconditioned_residual)
                    + (again.rz,)):
        assert torch.equal(a, b), "two runs differ"
    load(pcg, 0.0)  # pq == 0: alpha = 0
    keep = [f.clone() for f in pcg._x + pcg._r]
    pcg.update_step()
    for a, b in zip(keep, pcg._x + pcg._r):
        assert torch.equal(a, b)


def run_anisotropic(grid, device, rtol=1e-5):
    """The issue's solve: vertical weight 100, horizontal 1, periodic z,
    closed edges, float32.  Returns (PCG, CG) iteration counts."""
    k = weights(-100.0, 205.0, -100.0, h=-1.0)
    g = torch.Generator().manual_seed(5)
    b = torch.nn.functional.pad(torch.randn(8, 12, 14, generator=g),
                                (1, 1, 1, 1)).to(device)
    st = grid.make_stencil3d(b.shape, torch.float32, device, k,
                             z_boundary="periodic")
    x, info = st.make_cg("zline").solve(b, rtol=rtol, maxiter=400,
                                        check_every=1)
    _, plain = st.make_cg().solve(b, rtol=rtol, maxiter=400, check_every=1)
    assert info.converged and plain.converged
    (ax,) = oracle(grid, k, [x], "periodic")
    bi = interior(b.cpu().double(), 1)
    assert ((bi - ax).norm() / bi.norm()).item() <= 10 * rtol
    print("iterations: pcg", info.iterations, "cg", plain.iterations)
    assert 2 * info.iterations <= plain.iterations
    _, info0 = st.make_cg("zline").solve(b, rtol=rtol, maxiter=3,
                                         check_every=0)
    assert info0.converged is None and info0.iterations == 3
    assert isinstance(info0.residual_norm, torch.Tensor)
    return info.iterations, plain.iterations


@pytest.fixture(scope="module")
def grids():
    m.init()
    return {p: CartesianGrid(dims=(1, 1), periodic=p) for p in PERIODIC}


@pytest.mark.parametrize("dtype", F32_F64)
@pytest.mark.parametrize("zb,nz", SOLVE_CASES)
def test_line_solve_matches_dense(grids, zb, nz, dtype):
    print("err / (eps kappa):", run_solve(grids, zb, nz, dtype, "cpu")[0])


@pytest.mark.parametrize("zb", ZB)
def test_diagonal_power_of_two_is_exact(grids, zb, device="cpu"):
    r = int_data((2, 3, 9, 10), torch.float32, 3, device)
    st = grids[(True, True)].make_stencil3d(
        r.shape, torch.float32, device, weights(0.0, 4.0, 0.0),
        z_boundary=zb)
    z = st.make_line_solver().solve(r)
    assert torch.equal(interior(z, 1), interior(r, 1) / 4.0)


@pytest.mark.parametrize("dtype", F32_F64)
@pytest.mark.parametrize("zb", ZB)
def test_update_matches_composition(grids, zb, dtype):
    run_update(grids[(True, True)], zb, dtype, "cpu")


def test_pcg_halves_the_iterations(grids):
    run_anisotropic(grids[(False, False)], "cpu")


def test_errors(grids):
    grid = grids[(True, True)]

    def make(k, dtype=torch.float32, nz=5):
        return grid.make_stencil3d((nz, 9, 10), dtype, "cpu", k)

    penta = torch.zeros(5, 3, 3, dtype=torch.float64)
    penta[2, 1, 1], penta[0, 1, 1], penta[4, 1, 1] = 4.0, -1.0, -1.0
    with pytest.raises(ValueError, match="2, 0, 0"):
        make(penta).make_line_solver()
    for bad in (weights(-1.0, 1.0, -1.0), weights(0.0, -2.0, 0.0)):
        with pytest.raises(ValueError, match="not positive definite along z"):
            make(bad).make_line_solver()
    with pytest.raises(TypeError, match="float32 and float64"):
        make(weights(*BANDS), torch.bfloat16).make_line_solver()
    st = make(weights(*BANDS))
    with pytest.raises(ValueError, match="preconditioner"):
        st.make_cg("jacobi")
    for bad in (-1, 6, True, 2.0):
        with pytest.raises(ValueError, match="_lds_planes"):
            st.make_line_solver(_lds_planes=bad)
    assert type(st.make_cg()) is StencilCG
