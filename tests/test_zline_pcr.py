"""CPU suite for ``make_line_solver(method="pcr")`` and
``make_cg("zline", line_method="pcr")``, and the two runners it shares with
tests/test_gpu_zline_pcr.py.  Reference and bound are those of
tests/test_zline_pcg.py (``check_solution``): a level adds two products to
a value, ``ceil(log2 nz)`` levels against the march's ``2 nz`` dependent
steps, so the bound that holds the march holds the reduction.  ``nz`` in
(1, 2, 3, 7, 9, 33): no level, one level, non-powers of two.
"""

import math

import pytest
import torch

import mpi4jax_amd as m
from mpi4jax_amd.parallel.grid import CartesianGrid
from test_halo_adjoint import int_data
from test_halo_stencil import as_tuple, interior
from test_zline_pcg import (BANDS, F32_F64, PCG_CASES, WEAK, ZB,
                            check_solution, dense_t, weights)

NZS = (1, 2, 3, 7, 9, 33)
SOLVE_CASES = [(zb, nz, BANDS) for zb in ZB for nz in NZS
               if zb == "zero" or nz >= 3] + [(zb, 33, WEAK) for zb in ZB]


def run_pcr_solve(grid, zb, dtype, shape, bands, device, w=1, nf=1,
                  cols=None):
    """``solve`` on random data against the dense reference, and the
    tables' shape; returns the solver, the inputs and the outputs."""
    st = grid.make_stencil3d(shape, dtype, device, weights(*bands, w=w),
                             nfields=nf, z_boundary=zb)
    ls = st.make_line_solver("pcr", _pcr_columns=cols)
    assert (ls.method, ls.bands, ls.lds_planes) == ("pcr", bands, st.nz)
    assert ls.levels == math.ceil(math.log2(st.nz))
    assert ls.tables.shape == (2 * ls.levels + 2, st.nz)
    assert ls.tables.dtype == dtype and torch.isfinite(ls.tables).all()
    g = torch.Generator().manual_seed(sum(shape) + w)
    r = [torch.randn(shape, generator=g, dtype=torch.float64).to(dtype)
         .to(device) for _ in range(nf)]
    keep = [f.clone() for f in r]
    z = as_tuple(ls.solve(*r))
    t = dense_t(st.nz, *bands, zb)
    for fz, fr, fk in zip(z, r, keep):
        assert torch.equal(fr, fk), "solve() mutated its input"
        print("err / (eps kappa):", check_solution(
            fz, fr, t, dtype, (zb, shape, dtype, bands, cols), w))
    return ls, r, z


def run_pcr_update(grid, zb, dtype, shape, device, cols=None,
                   prep=lambda t: t):
    """One fused update under ``"pcr"`` against ``StencilCG.update_step``,
    the dense solve and ``dot``, on integer data (through ``prep``) with
    ``alpha = 2``; run twice, it is bitwise reproducible.  Returns the
    solver."""
    st = grid.make_stencil3d(shape, dtype, device, weights(*BANDS),
                             nfields=2, z_boundary=zb)
    kw = dict(line_method="pcr", _pcr_columns=cols)
    cg, pcg, again = st.make_cg(), st.make_cg("zline", **kw), \
        st.make_cg("zline", **kw)
    assert pcg.line_solver.method == "pcr"
    for s in (cg, pcg, again):
        for name, seed in (("_x", 1), ("_r", 2), ("_p", 3), ("_q", 4)):
            setattr(s, name, [prep(int_data(shape, dtype, seed + 10 * i,
                                            device)) for i in range(2)])
        s._rs.fill_(4.0), s._pq.fill_(2.0)
        s.update_step()
    for a, b in zip(cg._x + cg._r, pcg._x + pcg._r):
        assert torch.equal(interior(a, 1), interior(b, 1))
    assert pcg.rr.item() == sum(interior(f, 1).double().pow(2).sum().item()
                                for f in pcg._r)
    assert pcg.rz_old.item() == 4.0
    t = dense_t(shape[-3], *BANDS, zb)
    zs = as_tuple(pcg.preconditioned_residual)
    for fz, fr in zip(zs, pcg._r):
        check_solution(fz, fr, t, dtype, (zb, dtype, shape, cols))
    assert pcg.rz.item() == pytest.approx(st.dot(pcg._r, zs).item(),
                                          rel=1e-12)
    for a, b in zip(zs + (pcg.rz, pcg.rr),
                    as_tuple(again.preconditioned_residual)
                    + (again.rz, again.rr)):
        assert torch.equal(a, b), "two runs differ"
    return pcg


@pytest.fixture(scope="module")
def grid():
    m.init()
    return CartesianGrid(dims=(1, 1), periodic=(True, True))


@pytest.mark.parametrize("dtype", F32_F64)
@pytest.mark.parametrize("zb,nz,bands", SOLVE_CASES)
def test_pcr_solve_matches_dense(grid, zb, nz, bands, dtype):
    run_pcr_solve(grid, zb, dtype, (2, nz, 5, 14), bands, "cpu")


def test_pcr_errors(grid):
    def make(k=weights(*BANDS), dtype=torch.float32, nz=5):
        return grid.make_stencil3d((nz, 9, 10), dtype, "cpu", k)

    st = make()
    assert st.make_line_solver().method == "thomas"
    penta = torch.zeros(5, 3, 3, dtype=torch.float64)
    penta[2, 1, 1], penta[0, 1, 1], penta[4, 1, 1] = 4.0, -1.0, -1.0
    pcr = dict(method="pcr")
    # two float32 buffers of 128 planes x 64 columns are 64 KiB
    for exc, match, s, kw in [
            (ValueError, "method", st, dict(method="cyclic")),
            (ValueError, "_lds_planes", st, dict(pcr, _lds_planes=2)),
            (ValueError, "_pcr_columns", st, dict(_pcr_columns=8)),
            (ValueError, "_pcr_columns", make(nz=128),
             dict(pcr, _pcr_columns=64)),
            (ValueError, "largest nz of 511",
             make(dtype=torch.float64, nz=512), pcr),
            (ValueError, "2, 0, 0", make(penta), pcr),
            (ValueError, "not positive definite along z",
             make(weights(-1.0, 1.0, -1.0)), pcr),
            (ValueError, "not positive definite along z",
             make(weights(0.0, -2.0, 0.0)), pcr),
            (TypeError, "float32 and float64", make(dtype=torch.bfloat16),
             pcr)] + [(ValueError, "_pcr_columns", st,
                       dict(pcr, _pcr_columns=bad))
                      for bad in (0, 4, 12, 128, True, 8.0)]:
        with pytest.raises(exc, match=match):
            s.make_line_solver(**kw)
    with pytest.raises(ValueError, match="method"):
        st.make_cg("zline", line_method="cyclic")
    with pytest.raises(ValueError, match="preconditioner"):
        st.make_cg("jacobi", line_method="pcr")
    assert make(dtype=torch.float64, nz=511).make_line_solver(
        "pcr").columns_per_block == 8


@pytest.mark.parametrize("dtype", F32_F64)
@pytest.mark.parametrize("zb", ZB)
def test_pcr_update_matches_composition(grid, zb, dtype):
    run_pcr_update(grid, zb, dtype, (2, 7, 9, 14), "cpu")


def test_pcr_pcg_end_to_end(grid):
    """``PCG_CASES["a"]`` preconditioned through either method: the same
    ``M`` up to rounding, so ``"pcr"`` needs at most one iteration more."""
    dtype, zb, _, nf, shape, w, rtol = PCG_CASES["a"]
    k = weights(-100.0, 201.0 + 4 * w, -100.0, h=-1.0, w=w)
    g = torch.Generator().manual_seed(11)
    b = [torch.nn.functional.pad(
        interior(torch.randn(shape, generator=g, dtype=torch.float64), w),
        (w,) * 4).to(dtype) for _ in range(nf)]
    st = grid.make_stencil3d(shape, dtype, "cpu", k, nfields=nf,
                             z_boundary=zb)
    its = {}
    for method in ("thomas", "pcr"):
        _, info = st.make_cg("zline", line_method=method).solve(
            b, rtol=rtol, maxiter=200, check_every=1)
        assert info.converged is True, (method, info)
        its[method] = info.iterations
    print("iterations:", its)
    assert its["pcr"] <= its["thomas"] + 1
