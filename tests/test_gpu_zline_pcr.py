"""GPU suite for the cyclic-reduction line solve and its fused PCG update
(csrc/zline_pcr.hip, halo_zline_pcr_solve_nd / _update_nd) at world 1, on
the runners of tests/test_zline_pcr.py.  A block owns C cells of one row
and keeps P = 256 / C planes in flight.  Planes of (5 + 2w) x (68 + 2w)
make the host choose C = 64 and give a row two tiles, the second 4 cells
wide; (5, 14) makes it choose C = 16.  nz = 1 has no level; 7 / 9 / 33
leave a ragged last pass at P = 4 (C = 64) and P = 32 (C = 8).  ``EDGE``:
two buffers of nz x 64 fit in LDS up to nz = 127 (float32), 63 (float64).
"""

import pytest
import torch

import mpi4jax_amd as m
from mpi4jax_amd.parallel.grid import CartesianGrid
from test_gpu_zline_pcg import ring_fill_, ring_is
from test_halo_adjoint import int_data
from test_halo_stencil import as_tuple, interior
from test_zline_pcg import (BANDS, BENCH, F32_F64, ZB, _D, _F, case_id,
                            dense_t, kappa_inf, weights)
from test_zline_pcr import run_pcr_solve, run_pcr_update

pytestmark = pytest.mark.gpu

# (z boundary, shape, w, the host's C, dtype, bands); two fields if batched
PLANES = [((7, 70), 1, 64), ((9, 72), 2, 64), ((5, 14), 1, 16)]
EDGE = [(_D, 63, 64), (_D, 64, 32), (_F, 127, 64), (_F, 128, 32)]
CASES = [(zb, (nz,) + pl, w, c, dt, BANDS) for pl, w, c in PLANES
         for zb in ZB for nz in (1, 2, 7, 9, 33) if zb == "zero" or nz >= 3
         for dt in F32_F64]
CASES += [(zb, (2, 9, 7, 70), 1, 64, dt, BANDS) for zb in ZB
          for dt in F32_F64]
CASES += [(zb, (nz, 5, 70), 1, c, dt, BENCH) for zb in ZB
          for dt, nz, c in EDGE]
_CPU = {}  # case -> the CPU executor's outputs
NAN = float("nan")


@pytest.fixture(scope="module")
def grid():
    m.init()
    yield CartesianGrid(dims=(1, 1), periodic=(True, True))
    torch.cuda.synchronize()


@pytest.mark.parametrize("cols", (None, 8))
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_pcr_solve_matches_dense_and_cpu(grid, case, cols):
    zb, shape, w, c, dtype, bands = case
    args = (grid, zb, dtype, shape, bands)
    ls, _, got = run_pcr_solve(*args, "cuda", w, len(shape) - 2, cols)
    assert ls.columns_per_block == (cols or c)
    if case not in _CPU:
        _CPU[case] = run_pcr_solve(*args, "cpu", w, len(shape) - 2)[2]
    kappa = kappa_inf(dense_t(shape[-3], *bands, zb))
    for g, cpu in zip(got, _CPU[case]):
        assert ((g.cpu() - cpu).abs().max() / cpu.abs().max()
                <= 16 * torch.finfo(dtype).eps * kappa)


@pytest.mark.parametrize("dtype", F32_F64)
@pytest.mark.parametrize("zb", ZB)
def test_pcr_solve_does_not_depend_on_columns(grid, zb, dtype):
    """Every tile width runs the same instructions on a cell; a diagonal
    ``T`` with a power of two on it is exact."""
    args = (grid, zb, dtype, (9, 5, 70), BANDS, "cuda")
    narrow, wide = (run_pcr_solve(*args, cols=c)[2][0] for c in (8, 64))
    assert torch.equal(narrow, wide)
    st = grid.make_stencil3d((9, 5, 70), dtype, "cuda",
                             weights(0.0, 4.0, 0.0), z_boundary=zb)
    r = int_data((9, 5, 70), dtype, 3, "cuda")
    z = st.make_line_solver("pcr").solve(r)
    assert torch.equal(interior(z, 1), interior(r, 1) / 4.0)


@pytest.mark.parametrize("cols", (None, 8))
@pytest.mark.parametrize("dtype", F32_F64)
@pytest.mark.parametrize("zb", ZB)
def test_pcr_reads_and_writes_no_halo(grid, zb, dtype, cols):
    """NaN in every halo cell of the inputs and a sentinel in ``out``: the
    interiors, ``rr`` and ``rz`` are finite and bitwise those of the
    zero-halo run, and both rings are untouched.  The update runs through
    ``run_pcr_update``, so it is also the composition check at nz = 9."""
    w, shape = 2, (2, 9, 9, 72)
    st = grid.make_stencil3d(shape, dtype, "cuda", weights(*BANDS, w=w),
                             nfields=2, z_boundary=zb)
    g = torch.Generator().manual_seed(w)
    clean = [ring_fill_(torch.randn(shape, generator=g, dtype=torch.float64)
                        .to(dtype), w, 0.0).cuda() for _ in range(2)]
    ls = st.make_line_solver("pcr", _pcr_columns=cols)
    ref = as_tuple(ls.solve(*clean))
    bad = [ring_fill_(f.clone(), w, NAN) for f in clean]
    out = tuple(torch.full(shape, 7.0, dtype=dtype, device="cuda")
                for _ in range(2))
    for fg, fr, fb in zip(as_tuple(ls.solve(*bad, out=out)), ref, bad):
        assert torch.isfinite(interior(fg, w)).all(), "NaN read"
        assert torch.equal(interior(fg, w), interior(fr, w))
        assert ring_is(fg, w, 7.0) and ring_is(fb, w, NAN), "halo written"
    ref, got = (run_pcr_update(grid, zb, dtype, (2, 9, 7, 70), "cuda", cols,
                               lambda t: ring_fill_(t, 1, ring))
                for ring in (0.0, NAN))
    assert torch.equal(got.rr, ref.rr) and torch.equal(got.rz, ref.rz)
    for name in ("_z", "_x", "_r", "_p", "_q"):
        for a, b in zip(getattr(got, name), getattr(ref, name)):
            assert torch.equal(interior(a, 1), interior(b, 1)), name
            assert ring_is(a, 1, 0.0 if name == "_z" else NAN), name


@pytest.mark.parametrize("cols", (None, 8))
@pytest.mark.parametrize("dtype", F32_F64)
@pytest.mark.parametrize("zb", ZB)
def test_pcr_update_matches_composition(grid, zb, dtype, cols):
    run_pcr_update(grid, zb, dtype, (2, 33, 7, 70), "cuda", cols)


def test_pcr_bridge_refuses_before_its_launch(grid):
    """Each bad argument of the two bindings raises with the bridge's own
    message and leaves the sentinel-filled outputs alone."""
    from mpi4jax_amd._backend import rccl

    ext, shape = rccl.ext(), (128, 5, 70)
    ls = grid.make_stencil3d(shape, _F, "cuda", weights(*BANDS),
                             z_boundary="periodic").make_line_solver("pcr")
    names = ("levels", "nz", "ny", "nx", "width", "tables", "periodic",
             "cols")
    good = dict(zip(names, ls._geom()))
    assert good["cols"] == 32 and good["levels"] == 128
    tab = good["tables"]
    x, r, p, q = (int_data(shape, _F, s, "cuda") for s in (1, 2, 3, 4))
    z = torch.full(shape, 7.0, device="cuda")
    rz, pq, old, rr = (torch.full((), v, dtype=_D, device="cuda")
                       for v in (4.0, 2.0, 0.0, 0.0))
    keep = [t.clone() for t in (x, r)]

    def solve(**kw):
        a = {**good, "r": [r], "z": [z], **kw}
        ext.halo_zline_pcr_solve_nd(a["r"], a["z"], *(a[n] for n in names))

    def update(**kw):
        a = {**good, "z": [z], "rz": rz, "pq": pq, "rz_old": old, "rr": rr,
             "partials": ls._partials_buf(), **kw}
        ext.halo_zline_pcr_update_nd(
            [x], [r], [p], [q], a["z"], *(a[n] for n in names), a["rz"],
            a["pq"], a["rz_old"], a["rr"], a["partials"])

    cols_msg = "columns_per_block must be 8, 16, 32 or 64 and at most 63"
    tab_msg = r"tables must be a contiguous \(16, 128\) tensor"
    for call, exc, match, bad in [(c,) + b for c in (solve, update) for b in (
            (ValueError, cols_msg, dict(cols=48)),
            (ValueError, cols_msg, dict(cols=64)),
            (RuntimeError, tab_msg, dict(tables=tab.double())),
            (RuntimeError, tab_msg, dict(tables=tab[:-1].contiguous())),
            (RuntimeError, tab_msg, dict(tables=tab.cpu())),
            (RuntimeError, "nz = 127 does not divide 128 levels",
             dict(nz=127)),
            (ValueError, "overlaps", dict(z=[r])))] + [
            (update, RuntimeError, "at least 18 elements",
             dict(partials=ls._partials_buf()[:-1])),
            (update, ValueError, "rr overlaps written field 0",
             dict(rr=rz))]:
        with pytest.raises(exc, match=match):
            call(**bad)
    torch.cuda.synchronize()
    assert bool((z == 7.0).all()), "a refused call wrote z"
    assert torch.equal(x, keep[0]) and torch.equal(r, keep[1])
    assert (rz.item(), old.item(), rr.item()) == (4.0, 0.0, 0.0)
    solve()
    assert torch.equal(interior(z, 1), interior(ls.solve(r), 1))
