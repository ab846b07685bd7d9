"""GPU suite for the native per-column tridiagonal solves (csrc/ztridiag.hip
behind ztridiag_factor_nd / _solve_nd / _solve_bands_nd) at world 1, on the
runners, cases, reference and bound of tests/test_ztridiag.py.  The cases
cover the ragged second x tile, the y of planes 0 / 3 / all in LDS and
through the output (on the fused path cp through the workspace), and
ragged groups of right-hand sides at 1, 2 and 4 per thread.
"""

import pytest
import torch

import mpi4jax_amd as m
from mpi4jax_amd.parallel.grid import CartesianGrid
from test_halo_adjoint import int_data
from test_halo_stencil import interior
from test_zline_pcg import F32_F64, _D, _F, case_id
from test_ztridiag import (CASES, make_bands, rel_err, run_case, run_exact,
                           run_halo)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def grid():
    m.init()
    yield CartesianGrid(dims=(1, 1), periodic=(True, True))
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_solves_match_dense_and_cpu(grid, case):
    got, bound = run_case(grid, "cuda", case)
    for g, cpu in zip(got, run_case(grid, "cpu", case)[0]):
        assert rel_err(g, cpu.double()) <= bound


@pytest.mark.parametrize("dtype", F32_F64)
def test_results_do_not_depend_on_r_or_lds(grid, dtype):
    """Two fields of three batch columns at every ``_rhs_per_thread``, with
    0, 3 and all 7 planes in LDS: bitwise one result per path."""
    shape = (3, 7, 9, 72)
    bands = make_bands(*shape[1:], 4, device="cuda")
    r = [int_data(shape, dtype, s, "cuda") + 0.3 for s in (1, 2)]
    seen = []
    for rpt, lds in [(1, None), (2, None), (4, None), (4, 0), (1, 3), (2, 3),
                     (4, 3)]:
        ts = grid.make_tridiagonal_solver(
            shape, dtype, "cuda", *bands, nfields=2, width=2,
            _rhs_per_thread=rpt, _lds_planes=lds)
        assert (ts.rhs_per_thread, ts.lds_planes) == (rpt, 7 if lds is None
                                                      else lds)
        seen.append(ts.solve(*r) + ts.solve_bands(*bands, *r))
    for other in seen[1:]:
        for a, b in zip(seen[0], other):
            assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", F32_F64)
def test_diagonal_power_of_two_is_exact(grid, dtype):
    run_exact(grid, "cuda", dtype)


@pytest.mark.parametrize("rpt,lds", [(None, None), (4, 3), (1, 0)])
@pytest.mark.parametrize("dtype", F32_F64)
def test_reads_and_writes_no_halo(grid, dtype, rpt, lds):
    run_halo(grid, "cuda", dtype, rpt, lds)


def test_set_bands_refuses_a_bad_pivot(grid):
    """One interior pivot made non-positive at plane 2 is refused with the
    plane's number; the same defect in a halo cell is accepted."""
    shape = (7, 9, 72)
    lower, diag, upper = make_bands(*shape, 6, device="cuda")
    ts = grid.make_tridiagonal_solver(shape, _F, "cuda", lower, diag, upper,
                                      width=2)
    keep = ts.factors.clone()
    bad = diag.clone()
    bad[2, 5, 69] = -1.0
    with pytest.raises(ValueError,
                       match="not positive definite along z: pivot 2"):
        ts.set_bands(lower, bad, upper)
    assert torch.equal(ts.factors, keep)
    bad = diag.clone()
    bad[2, 1, 69] = -1.0
    ts.set_bands(lower, bad, upper)
    assert torch.equal(ts.factors, keep)


def test_bridge_refuses_before_its_launch(grid):
    """Each bad argument of the three bindings raises with the bridge's own
    message and leaves the sentinel-filled outputs alone."""
    from mpi4jax_amd._backend import rccl

    ext, shape, w = rccl.ext(), (2, 7, 9, 72), 2
    bands = make_bands(*shape[1:], 8, device="cuda")
    ts = grid.make_tridiagonal_solver(shape, _F, "cuda", *bands, width=w)
    r = int_data(shape, _F, 1, "cuda")
    x = torch.full(shape, 7.0, device="cuda")
    fac = torch.full_like(ts.factors, 7.0)
    status = torch.full((4, 2), 7.0, dtype=_D, device="cuda")
    work = torch.empty(0, device="cuda")
    alias, stacked = bands[1].clone(), torch.stack(bands)
    geom = dict(batch=2, nz=7, ny=9, nx=72, width=w, rpt=2, lds=7)
    names = tuple(geom)

    def factor(**kw):
        a = {**geom, "bands": bands, "factors": fac, "status": status, **kw}
        ext.ztridiag_factor_nd(*a["bands"], a["factors"], a["status"],
                               *(a[n] for n in names[1:5]))

    def solve(**kw):
        a = {**geom, "r": [r], "x": [x], "factors": ts.factors, **kw}
        ext.ztridiag_solve_nd(a["r"], a["x"], a["factors"],
                              *(a[n] for n in names))

    def fused(**kw):
        a = {**geom, "bands": bands, "r": [r], "x": [x], "work": work, **kw}
        ext.ztridiag_solve_bands_nd(*a["bands"], a["r"], a["x"], a["work"],
                                    *(a[n] for n in names))

    both = [(ValueError, "rhs_per_thread must be 1, 2 or 4", dict(rpt=3)),
            (ValueError, "non-empty interior", dict(width=5)),
            (ValueError, "elements, expected", dict(nz=6)),
            (RuntimeError, "differs in dtype", dict(x=[x.double()])),
            (RuntimeError, "on the GPU", dict(r=[r.cpu()])),
            (RuntimeError, "contiguous", dict(r=[r.transpose(0, 1)])),
            (ValueError, "1 right-hand side.s. but 2", dict(x=[x, x])),
            (ValueError, "overlaps", dict(x=[r]))]
    for call, exc, match, bad in [(c,) + b for c in (solve, fused)
                                  for b in both] + [
            (solve, ValueError, r"lds_planes must be in 0..min\(nz, 31\)",
             dict(lds=8)),
            (solve, RuntimeError, "factors must have the fields' dtype",
             dict(factors=ts.factors.double())),
            (solve, ValueError, "factors has", dict(factors=ts.factors[:2])),
            (fused, ValueError, r"lds_planes must be in 0..min\(nz, 12\)",
             dict(rpt=4, lds=16, nz=16,
                  bands=make_bands(16, 9, 72, 1, device="cuda"),
                  r=[torch.zeros(32, 9, 72, device="cuda")],
                  x=[torch.full((32, 9, 72), 7.0, device="cuda")])),
            (fused, ValueError, "work has", dict(lds=3)),
            (fused, RuntimeError, "dtype and device of lower",
             dict(bands=(bands[0], bands[1].float(), bands[2]))),
            (fused, ValueError, "a band overlaps", dict(
                bands=(bands[0], alias, bands[2]),
                x=[alias.view(_F).view(shape)])),
            (factor, ValueError, "diag has", dict(
                bands=(bands[0], bands[1][:6], bands[2]))),
            (factor, RuntimeError, "status must be", dict(
                status=status[:3])),
            (factor, RuntimeError, "status must be", dict(
                status=status.float())),
            (factor, ValueError, "factors has", dict(factors=fac[:2])),
            (factor, ValueError, "overlaps", dict(
                bands=tuple(stacked), factors=stacked))]:
        with pytest.raises(exc, match=match):
            call(**bad)
    torch.cuda.synchronize()
    for t in (x, fac, status):
        assert bool((t == 7.0).all()), "a refused call wrote"
    solve(), factor()
    assert torch.equal(interior(x, w), interior(ts.solve(r), w))
    assert torch.equal(interior(fac, w), interior(ts.factors, w))
