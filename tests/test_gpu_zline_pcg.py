"""GPU suite for the native line solve and the fused PCG update
(csrc/zline.hip + bridge.cpp:halo_zline_solve_nd / _pcg_update_nd) at world
1.  References, bounds and cases are those of tests/test_zline_pcg.py.
``_lds_planes`` in (0, 3, None): at nz = 7 the value 3 splits a column
between the LDS stash and the stash in ``z``.  The kernel's tile is 4 rows
x 64 columns, so (2, nz, 41, 70) spans 10 x 2 ragged tiles per column.

``TALL_CASES`` x ``TALL_LDS`` = (0, 32, None), 32 clipped to what the dtype
allows: the sweeps run in batches of ``kZU = 4`` planes, and the default
stash is 63 float32 or 31 float64 planes (64512 or 63488 B of dynamic LDS
next to the update's 32 B of static ``wave_sums``).  So None at nz = 63
(float32) and 31 (float64) is the largest all-LDS launch; at 64 and 32 one
plane goes through ``z``, 64 in float32 being the benchmark's launch; at 65
and 33 the default split meets a ragged last batch.  32 puts the stash
boundary on a batch edge, where 31, 63 and 3 do not, and 0 sends every
plane through ``z``.  The planes are (5 + 2w) x (68 + 2w) at w in 1..3:
2 x 2 tiles, ragged both ways, whose origin is ``w`` and not 1.  The
poisoned-halo tests fill every cell outside that interior with NaN, so a
column, a tile or a plane read one cell too far shows as a NaN or as a
changed sentinel; the refusal tests call the two bindings with one bad
argument at a time, none of which gets as far as a launch.
"""

import pytest
import torch

import mpi4jax_amd as m
from mpi4jax_amd.parallel.grid import CartesianGrid
from test_gpu_halo_exchanger import OPEN
from test_halo_adjoint import int_data
from test_halo_stencil import as_tuple, interior
from test_zline_pcg import (BANDS, F32_F64, PCG_CASES, SOLVE_CASES,
                            TALL_CASES, UPDATE_CASES, ZB, case_id, clip_lds,
                            dense_t, kappa_inf, run_anisotropic, run_pcg,
                            run_solve, run_tall, run_update,
                            test_diagonal_power_of_two_is_exact as exact,
                            weights)

pytestmark = pytest.mark.gpu

LDS = (0, 3, None)
TALL_LDS = (0, 32, None)
_CPU_TALL = {}  # row of TALL_CASES -> the CPU executor's outputs


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


@pytest.mark.parametrize("lds", TALL_LDS)
@pytest.mark.parametrize("row", range(len(TALL_CASES)),
                         ids=lambda i: case_id(TALL_CASES[i]))
def test_tall_wide_line_solve_matches_dense_and_cpu(grids, row, lds):
    case = TALL_CASES[row]
    zb, nz, _, dtype, bands, _ = case
    worst, got = run_tall(grids[(True, True)], case, "cuda", lds)
    print("err / (eps kappa):", worst)
    if row not in _CPU_TALL:
        _CPU_TALL[row] = run_tall(grids[(True, True)], case, "cpu")[1]
    kappa = kappa_inf(dense_t(nz, *bands, zb))
    for g, c in zip(got, _CPU_TALL[row]):
        assert ((g - c).abs().max() / c.abs().max()
                <= 16 * torch.finfo(dtype).eps * kappa)


@pytest.mark.parametrize("lds", TALL_LDS)
@pytest.mark.parametrize("zb", ZB)
@pytest.mark.parametrize("shape,w,dtype", UPDATE_CASES, ids=case_id)
def test_update_matches_composition_at_height(grids, shape, w, dtype, zb,
                                              lds):
    run_update(grids[(True, True)], zb, dtype, "cuda",
               clip_lds(lds, shape[-3], dtype), shape, w)


def ring_fill_(t, w, value):
    """Every cell of ``t`` outside the interior at width ``w`` = value."""
    keep = interior(t, w).clone()
    t.fill_(value)
    interior(t, w).copy_(keep)
    return t


def ring_is(t, w, value):
    """The ring of ``t`` holds ``value`` (NaN: is NaN) in every cell."""
    mask = torch.ones_like(t, dtype=torch.bool)
    interior(mask, w).fill_(False)
    ring = t[mask]
    return bool((ring.isnan() if value != value else ring == value).all())


@pytest.mark.parametrize("dtype", F32_F64)
@pytest.mark.parametrize("zb", ZB)
@pytest.mark.parametrize("w", (1, 2))
def test_solve_reads_and_writes_no_halo(grids, w, zb, dtype):
    """NaN in every halo cell of ``r`` and a sentinel in ``out``: the
    interior is finite and bitwise that of a zero halo, the ring of
    ``out`` keeps the sentinel."""
    shape = (2, 9, 7 + 2 * (w - 1), 70 + 2 * (w - 1))
    st = grids[(True, True)].make_stencil3d(
        shape, dtype, "cuda", weights(*BANDS, w=w), nfields=2, z_boundary=zb)
    g = torch.Generator().manual_seed(w)
    clean = [ring_fill_(torch.randn(shape, generator=g, dtype=torch.float64)
                        .to(dtype), w, 0.0).cuda() for _ in range(2)]
    for lds in (0, 4, None):
        ls = st.make_line_solver(_lds_planes=lds)
        ref = as_tuple(ls.solve(*clean))
        bad = [ring_fill_(f.clone(), w, float("nan")) for f in clean]
        out = tuple(torch.full(shape, 7.0, dtype=dtype, device="cuda")
                    for _ in range(2))
        got = as_tuple(ls.solve(*bad, out=out))
        for fg, fr, fb in zip(got, ref, bad):
            assert torch.isfinite(interior(fg, w)).all(), (lds, "NaN read")
            assert torch.equal(interior(fg, w), interior(fr, w)), lds
            assert ring_is(fg, w, 7.0), (lds, "halo of out written")
            assert ring_is(fb, w, float("nan")), (lds, "halo of r written")


@pytest.mark.parametrize("dtype", F32_F64)
@pytest.mark.parametrize("zb", ZB)
@pytest.mark.parametrize("w", (1, 2))
def test_update_reads_and_writes_no_halo(grids, w, zb, dtype):
    """NaN in every halo cell of x, r, p and q: ``rr``, ``rz``, z and the
    interiors are bitwise those of the zero-halo run, the rings stay
    NaN."""
    shape = (2, 9, 7 + 2 * (w - 1), 70 + 2 * (w - 1))
    st = grids[(True, True)].make_stencil3d(
        shape, dtype, "cuda", weights(*BANDS, w=w), nfields=2, z_boundary=zb)
    names = ("_x", "_r", "_p", "_q")

    def run(lds, ring):
        s = st.make_cg("zline", _lds_planes=lds)
        for name, seed in zip(names, range(1, 5)):
            setattr(s, name, [ring_fill_(
                int_data(shape, dtype, seed + 10 * i, "cuda"), w, ring)
                for i in range(2)])
        s._rs.fill_(4.0), s._pq.fill_(2.0)
        s.update_step()
        return s

    for lds in (0, 4, None):
        ref, got = run(lds, 0.0), run(lds, float("nan"))
        assert torch.equal(got.rr, ref.rr) and torch.equal(got.rz, ref.rz)
        assert got.rr.item() > 0 and got.rz.item() == got.rz.item()
        for a, b in zip(got._z, ref._z):
            assert torch.equal(a, b), (lds, "z differs")
        for name in names:
            for a, b in zip(getattr(got, name), getattr(ref, name)):
                assert torch.equal(interior(a, w), interior(b, w)), (lds,
                                                                     name)
                assert ring_is(a, w, float("nan")), (lds, name, "halo")


def test_bridge_refuses_before_its_launch(grids):
    """Each bad argument of the two bindings raises with the bridge's own
    message and leaves the sentinel-filled outputs alone.  The aliasing
    checks are the Krylov layer's, which raise ValueError as every
    "overlaps" refusal of this project does."""
    from mpi4jax_amd._backend import rccl

    ext, shape, nz = rccl.ext(), (65, 7, 70), 65
    st = grids[(True, True)].make_stencil3d(
        shape, torch.float32, "cuda", weights(*BANDS), z_boundary="periodic")
    ls = st.make_line_solver()
    names = ("levels", "nz", "ny", "nx", "width", "tables", "periodic",
             "lds_planes")
    good = dict(zip(names, ls._geom()))
    assert good["lds_planes"] == 63 and good["levels"] == nz
    tab = good["tables"]
    r = torch.randn(shape, device="cuda")
    z = torch.full(shape, 7.0, device="cuda")

    def solve(**kw):
        a = dict(good, r=[r], z=[z])
        a.update(kw)
        ext.halo_zline_solve_nd(a.pop("r"), a.pop("z"),
                                *(a[n] for n in names))

    solve()
    assert torch.equal(interior(z, 1), interior(ls.solve(r), 1))
    z.fill_(7.0)
    lds_msg = r"lds_planes must be in 0\.\.min\(nz, 63\)"
    tab_msg = r"tables must be a contiguous \(4, 65\) tensor"
    for exc, match, bad in (
            (ValueError, lds_msg, dict(lds_planes=nz + 1)),
            (ValueError, lds_msg, dict(lds_planes=-1)),
            (ValueError, lds_msg, dict(lds_planes=64)),
            (RuntimeError, tab_msg, dict(tables=tab.double())),
            (RuntimeError, tab_msg,
             dict(tables=tab[:, :nz - 1].contiguous())),
            (RuntimeError, tab_msg, dict(tables=tab.cpu())),
            (RuntimeError, "nz = 64 does not divide 65 levels", dict(nz=64)),
            (ValueError, "written field 0 overlaps read field 0",
             dict(r=[z]))):
        with pytest.raises(exc, match=match):
            solve(**bad)
    torch.cuda.synchronize()
    assert bool((z == 7.0).all()), "a refused solve wrote z"

    x, p, q = (int_data(shape, torch.float32, s, "cuda") for s in (1, 3, 4))
    keep = [t.clone() for t in (x, r)]
    rz, pq, old, rr = (torch.full((), v, dtype=torch.float64, device="cuda")
                       for v in (4.0, 2.0, 0.0, 0.0))
    part = ls._partials_buf()

    def update(**kw):
        a = dict(good, rz=rz, pq=pq, rz_old=old, rr=rr, partials=part)
        a.update(kw)
        ext.halo_zline_pcg_update_nd(
            [x], [r], [p], [q], [z], *(a[n] for n in names), a["rz"],
            a["pq"], a["rz_old"], a["rr"], a["partials"])

    with pytest.raises(RuntimeError, match="partials must be a contiguous "
                       "float64 tensor of at least 8 elements"):
        update(partials=part[:-1])
    with pytest.raises(ValueError, match="rr overlaps written field 0"):
        update(rr=rz)
    torch.cuda.synchronize()
    assert bool((z == 7.0).all()), "a refused update wrote z"
    assert torch.equal(x, keep[0]) and torch.equal(r, keep[1])
    assert (rz.item(), old.item(), rr.item()) == (4.0, 0.0, 0.0)


@pytest.mark.parametrize("name", PCG_CASES)
def test_pcg_end_to_end(grids, name):
    """Both devices run the same recurrence on the same tables and differ
    by FMA contraction alone: the iteration counts are within 1."""
    cpu = run_pcg(grids, name, "cpu")
    assert abs(run_pcg(grids, name, "cuda") - cpu) <= 1


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
