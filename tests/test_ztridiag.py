"""CPU suite for ``CartesianGrid.make_tridiagonal_solver``
(parallel/ztridiag.ColumnTridiagonal) and the runners it shares with
tests/test_gpu_ztridiag.py.

Bands: seeded, float64, ``lower``, ``upper`` in ``-U(0.2, 1)`` and ``diag =
|lower| + |upper| + U(0.1, 1)``: row diagonal dominance keeps every pivot
positive, and ``lower != upper``.  Reference: the dense float64 ``T`` of
every interior column and ``torch.linalg.solve``.  Bound: the line solves'
own (tests/test_zline_pcg.py), max error over max reference ``<= 16 eps
kappa_inf``, with the largest ``kappa_inf`` over the case's columns.

Shapes: interior planes of 5 x 68 (two x tiles, the second 4 cells wide,
ragged against the 4-row tile) and 5 x 12; halo widths 0 and 2; nz of 1, 2
and 7; 0, 3 or all planes in LDS; 1, 3 and 6 right-hand sides against 1, 2
and 4 per thread (ragged groups of 3 in 4 and 4 + 2); float32 bands under
either field dtype.
"""

import pytest
import torch

import mpi4jax_amd as m
from mpi4jax_amd.parallel.grid import CartesianGrid
from test_gpu_zline_pcg import ring_fill_, ring_is
from test_halo_adjoint import int_data
from test_halo_stencil import as_tuple, interior
from test_zline_pcg import F32_F64, _D, _F, case_id, kappa_inf

WIDE, SMALL = (5, 68), (5, 12)
# (plane, w, nz, _lds_planes, nfields, batch, _rhs_per_thread, dtype, bands)
CASES = [(WIDE, 0, nz, None, 1, (), None, dt, _D)
         for nz in (1, 2, 7) for dt in F32_F64]
CASES += [(SMALL, 2, 7, None, nf, (3,), r, dt, _D) for nf, r, dt in (
    (1, 1, _F), (1, 2, _D), (1, 4, _F), (2, 1, _D), (2, 2, _F), (2, 4, _D))]
CASES += [(WIDE, 2, 7, lds, 2, (3,), r, dt, _D) for lds, r, dt in (
    (0, 4, _F), (0, 4, _D), (3, 4, _F), (3, 4, _D), (0, 1, _F), (3, 2, _D))]
CASES += [(SMALL, 0, 7, None, 1, (), None, dt, _F) for dt in F32_F64]
NAN = float("nan")


def make_bands(nz, ny, nx, seed, dtype=_D, device="cpu"):
    g = torch.Generator().manual_seed(seed)

    def uniform(a, b):
        return a + (b - a) * torch.rand((nz, ny, nx), generator=g, dtype=_D)

    lower, upper = -uniform(0.2, 1.0), -uniform(0.2, 1.0)
    diag = lower.abs() + upper.abs() + uniform(0.1, 1.0)
    return tuple(b.to(dtype).to(device) for b in (lower, diag, upper))


def dense(bands, w):
    """``T`` of every interior column, ``(columns, nz, nz)`` in float64."""
    lo, d, up = (interior(b.cpu().double(), w).flatten(1).T for b in bands)
    return (torch.diag_embed(d) + torch.diag_embed(lo[:, 1:], -1)
            + torch.diag_embed(up[:, :-1], 1))


def rel_err(got, ref):
    return ((got.cpu().double() - ref).abs().max() / ref.abs().max()).item()


def run_case(grid, device, case):
    """``solve`` and ``solve_bands`` on random data against the dense
    reference; returns the outputs of ``solve`` and the bound."""
    plane, w, nz, lds, nf, batch, rpt, dtype, bdt = case
    ny, nx = plane[0] + 2 * w, plane[1] + 2 * w
    shape = batch + (nz, ny, nx)
    bands = make_bands(nz, ny, nx, sum(shape), bdt, device)
    ts = grid.make_tridiagonal_solver(
        shape, dtype, device, *bands, nfields=nf, width=w,
        _rhs_per_thread=rpt, _lds_planes=lds)
    assert ts.factors.shape == (3, nz, ny, nx) and ts.factors.dtype == dtype
    assert ts.rhs_per_thread == (rpt or 1)
    assert ts.lds_planes == (nz if lds is None else lds)
    g = torch.Generator().manual_seed(nz + w)
    r = [torch.randn(shape, generator=g, dtype=_D).to(dtype).to(device)
         for _ in range(nf)]
    keep = [f.clone() for f in r]
    solved = as_tuple(ts.solve(*r))
    fused = as_tuple(ts.solve_bands(*bands, *r))
    t = dense(bands, w)
    bound = 16 * torch.finfo(dtype).eps * kappa_inf(t).max().item()
    for fs, ff, fr, fk in zip(solved, fused, r, keep):
        assert torch.equal(fr, fk), "a solve mutated its input"
        assert torch.equal(fs, ff), "solve_bands is not set_bands + solve"
        assert ring_is(fs, w, 0.0), "a new output has a zero halo"
        rhs = interior(fr.cpu().double(), w).reshape(-1, nz, t.shape[0])
        ref = torch.linalg.solve(t, rhs.transpose(1, 2)[..., None])
        got = interior(fs, w).reshape(-1, nz, t.shape[0]).transpose(1, 2)
        err = rel_err(got, ref[..., 0])
        print("err / bound:", err / bound)
        assert err <= bound, (case, err, bound)
    return solved, bound


def run_exact(grid, device, dtype):
    """A diagonal ``T`` of powers of two divides exactly."""
    shape, w = (2, 7, 9, 72), 2
    diag = torch.ldexp(torch.ones(shape[1:], dtype=_D),
                       int_data(shape[1:], torch.int32, 5)).to(device)
    zero = torch.zeros_like(diag)
    ts = grid.make_tridiagonal_solver(shape, dtype, device, zero, diag, zero,
                                      width=w)
    r = int_data(shape, dtype, 3, device)
    for x in (ts.solve(r), ts.solve_bands(zero, diag, zero, r)):
        assert torch.equal(interior(x, w), interior(r / diag.to(dtype), w))


def run_halo(grid, device, dtype, rpt=None, lds=None):
    """NaN in every halo cell of the right-hand sides and of the bands and
    a sentinel in ``out``: the interiors are finite and bitwise those of
    the clean run, no ring is written, ``.factors`` has a zero halo."""
    w, shape = 2, (3, 7, 9, 72)
    kw = dict(nfields=2, width=w, _rhs_per_thread=rpt, _lds_planes=lds)
    bands = make_bands(*shape[1:], 9, device=device)
    g = torch.Generator().manual_seed(w)
    clean = [ring_fill_(torch.randn(shape, generator=g, dtype=_D).to(dtype),
                        w, 0.0).to(device) for _ in range(2)]
    ref = grid.make_tridiagonal_solver(shape, dtype, device, *bands,
                                       **kw).solve(*clean)
    nb = [ring_fill_(b.clone(), w, NAN) for b in bands]
    bad = [ring_fill_(f.clone(), w, NAN) for f in clean]
    keep = [t.clone() for t in nb + bad]
    ts = grid.make_tridiagonal_solver(shape, dtype, device, *nb, **kw)
    assert ring_is(ts.factors, w, 0.0)
    assert torch.isfinite(interior(ts.factors, w)).all()
    for call in (ts.solve, lambda *f, out: ts.solve_bands(*nb, *f, out=out)):
        out = tuple(torch.full(shape, 7.0, dtype=dtype, device=device)
                    for _ in range(2))
        for fg, fr in zip(call(*bad, out=out), ref):
            assert torch.isfinite(interior(fg, w)).all(), "NaN read"
            assert torch.equal(interior(fg, w), interior(fr, w))
            assert ring_is(fg, w, 7.0), "halo written"
    for a, b in zip(nb + bad, keep):
        assert ring_is(a, w, NAN), "input ring written"
        assert torch.equal(interior(a, w), interior(b, w)), "input mutated"


@pytest.fixture(scope="module")
def grid():
    m.init()
    return CartesianGrid(dims=(1, 1), periodic=(True, True))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_solves_match_dense(grid, case):
    run_case(grid, "cpu", case)


@pytest.mark.parametrize("dtype", F32_F64)
def test_diagonal_power_of_two_is_exact(grid, dtype):
    run_exact(grid, "cpu", dtype)


@pytest.mark.parametrize("dtype", F32_F64)
def test_reads_and_writes_no_halo(grid, dtype):
    run_halo(grid, "cpu", dtype)


def test_refusals(grid):
    shape = (2, 4, 6, 8)
    bands = make_bands(4, 6, 8, 1)

    def make(shape=shape, dtype=_F, bands=bands, **kw):
        return grid.make_tridiagonal_solver(shape, dtype, "cpu", *bands, **kw)

    def holed(j, i):
        d = bands[1].clone()
        d[2, j, i] = -1.0
        return bands[0], d, bands[2]

    for exc, match, kw in [
            (ValueError, "nz, ny, nx", dict(shape=(6, 8))),
            (ValueError, "diag has shape",
             dict(bands=(bands[0], bands[1][:3], bands[2]))),
            (ValueError, "empty interior", dict(width=3)),
            (ValueError, "width", dict(width=-1)),
            (ValueError, "width", dict(width=1.0)),
            (ValueError, "nfields", dict(nfields=0)),
            (ValueError, "nfields", dict(nfields=True)),
            (ValueError, "_rhs_per_thread", dict(_rhs_per_thread=3)),
            (ValueError, "_lds_planes", dict(_lds_planes=5)),
            (TypeError, "upper must be float32 or float64",
             dict(bands=(bands[0], bands[1], bands[2].to(torch.complex64)))),
            (TypeError, "lower must be float32 or float64",
             dict(bands=(bands[0].long(), bands[1], bands[2]))),
            (TypeError, "float32 and float64", dict(dtype=torch.bfloat16)),
            (ValueError, "not positive definite along z: pivot 2",
             dict(bands=holed(3, 4), width=1))]:
        with pytest.raises(exc, match=match):
            make(**kw)
    ts = make(bands=holed(0, 4), width=1)  # the same defect in the halo
    assert torch.isfinite(ts.factors).all()
    assert (ts.rhs_per_thread, make(nfields=2).rhs_per_thread) == (2, 4)
    with pytest.raises(ValueError, match="not positive definite along z"):
        ts.set_bands(*holed(1, 1))
    r = torch.ones(shape)
    for match, args, kw in [
            ("built for 1 field", (r, r), {}),
            ("right-hand side 0", (r[0],), {}),
            ("right-hand side 0", (r.double(),), {}),
            ("right-hand side 0", (r.to("meta"),), {}),
            ("contiguous", (r.transpose(-1, -2).contiguous()
                            .transpose(-1, -2),), {}),
            (r"out\[0\] overlaps input 0", (r,), dict(out=r)),
            ("output 0", (r,), dict(out=r[0]))]:
        with pytest.raises(ValueError, match=match):
            ts.solve(*args, **kw)
        with pytest.raises(ValueError, match=match):
            ts.solve_bands(*bands, *args, **kw)
