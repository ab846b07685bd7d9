"""CPU suite for parallel/zline.ZLineSolver and parallel/pcg.StencilPCG, and
the checks it shares with tests/test_gpu_zline_pcg.py.

Reference of a line solve: the dense float64 ``T`` and
``torch.linalg.solve`` along z.  Bound: ``|z - z_ref|_inf / |z_ref|_inf <=
16 eps kappa_inf(T)``.  LU of a diagonally dominant tridiagonal has
``|L||U| <= 3 |T|`` and the solve ``f(u) ~ 4u``, which gives ``6 eps
kappa``; the rest is margin for the rounded reciprocal tables.  The bands
``(-1.5, 3, -1)`` are diagonally dominant and not symmetric, so a swap of
``a`` and ``c`` shows.

``TALL_CASES`` are the heights at which the native kernel (block of 4 rows
x 64 columns, sweeps in batches of ``kZU = 4`` planes, at most 63 float32
or 31 float64 planes of LDS stash) changes path: nz = 8 / 9 is two full
batches and one plane more; 31 (float64) and 63 (float32) are the largest
all-LDS launches; 32 and 64 put one plane through ``z`` (64 in float32 is
the benchmark's launch) and end the column on a batch edge; 33 and 65 split
the stash by default and have a ragged last batch.  Their planes are
(5 + 2w) x (68 + 2w): 2 x 2 tiles, ragged both ways, at halo width w in
1..3, so an origin or a tile grid offset by 1 instead of ``w`` lands in the
halo.  The bands are ``BANDS``, the benchmark's ``(-100, 205, -100)`` and
the weakly dominant ``(-1, 2.01, -1)`` (kappa of order 1e2 to 1e3).
``UPDATE_CASES`` take the fused update to the same heights and to w = 2,
and ``PCG_CASES`` run whole solves over two fields and two columns, a
default split under periodic z, and w = 2.
"""

import pytest
import torch

import mpi4jax_amd as m
from mpi4jax_amd.parallel import StencilCG, StencilPCG, ZLineSolver, zline
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
BENCH = (-100.0, 205.0, -100.0)
WEAK = (-1.0, 2.01, -1.0)
_Z, _P, _F, _D = "zero", "periodic", torch.float32, torch.float64
# (z boundary, nz, w, dtype, bands, batch): every nz at w = 1, every w at
# nz = 33 and 65; batch = 2 runs two fields of (2, nz, ..) once per dtype
TALL_CASES = [
    (_Z, 8, 1, _F, BANDS, 0), (_P, 8, 1, _D, BENCH, 0),
    (_P, 9, 1, _F, WEAK, 0), (_Z, 9, 1, _D, BANDS, 0),
    (_Z, 31, 1, _D, BENCH, 0), (_P, 31, 1, _D, BANDS, 0),
    (_P, 31, 1, _F, WEAK, 0),
    (_P, 32, 1, _D, WEAK, 0), (_Z, 32, 1, _F, BANDS, 0),
    (_Z, 33, 1, _D, BANDS, 0), (_P, 33, 1, _D, BENCH, 0),
    (_Z, 33, 1, _F, WEAK, 0),
    (_Z, 63, 1, _F, BENCH, 0), (_P, 63, 1, _F, BANDS, 0),
    (_Z, 63, 1, _D, WEAK, 0),
    (_P, 64, 1, _F, BENCH, 0), (_Z, 64, 1, _F, BANDS, 0),
    (_P, 64, 1, _D, WEAK, 0),
    (_Z, 65, 1, _F, WEAK, 0), (_P, 65, 1, _F, BANDS, 0),
    (_P, 65, 1, _D, BENCH, 0),
    (_P, 33, 2, _D, BANDS, 0), (_Z, 33, 2, _F, BENCH, 0),
    (_Z, 65, 2, _F, BANDS, 0), (_P, 65, 2, _D, WEAK, 0),
    (_Z, 33, 3, _D, WEAK, 0), (_P, 33, 3, _F, BANDS, 0),
    (_P, 65, 3, _F, BENCH, 0), (_Z, 65, 3, _D, BANDS, 0),
    (_P, 65, 2, _F, BANDS, 2), (_Z, 33, 1, _D, BENCH, 2),
]
# (shape, w, dtype) of the fused update beyond run_update's default
UPDATE_CASES = [((2, 33, 7, 70), 1, _D), ((2, 65, 7, 70), 1, _F),
                ((2, 9, 9, 72), 2, _F), ((2, 9, 9, 72), 2, _D)]
# name: (dtype, z boundary, grid, fields, shape, w, rtol)
PCG_CASES = {
    "a": (_D, _Z, (True, True), 2, (2, 9, 14, 70), 1, 1e-10),
    "b": (_F, _P, (False, True), 1, (33, 7, 70), 1, 1e-5),
    "c": (_F, _Z, (False, False), 1, (9, 11, 74), 2, 1e-5),
}
SINGULAR = ((-1.0, 2.0, -1.0), (-0.5, 1.0, -0.5), (-100.0, 200.0, -100.0))
NEARLY = (-1.0, 2.0 + 1e-6, -1.0)


def case_id(v):
    if isinstance(v, torch.dtype):
        return str(v)[6:]
    if isinstance(v, tuple):
        return "x".join(case_id(e) or str(e) for e in v)
    return None


def weights(a, b, c, h=-0.25, w=1):
    """Bands ``(a, b, c)`` along z and ``h`` on the in-plane star out to
    distance ``w``: a 3 x (2w+1) x (2w+1) table, halo width ``w``."""
    k = torch.zeros(3, 2 * w + 1, 2 * w + 1, dtype=torch.float64)
    k[0, w, w], k[1, w, w], k[2, w, w] = a, b, c
    for d in range(1, w + 1):
        k[1, w - d, w] = k[1, w + d, w] = k[1, w, w - d] = k[1, w, w + d] = h
    return k


def dense_t(nz, a, b, c, zb):
    t = (torch.diag(torch.full((nz,), b, dtype=torch.float64))
         + torch.diag(torch.full((nz - 1,), a, dtype=torch.float64), -1)
         + torch.diag(torch.full((nz - 1,), c, dtype=torch.float64), 1))
    if zb == "periodic":
        t[0, nz - 1] += a
        t[nz - 1, 0] += c
    return t


def kappa_inf(t):
    return (torch.linalg.matrix_norm(t, float("inf"))
            * torch.linalg.matrix_norm(torch.linalg.inv(t), float("inf")))


def clip_lds(lds, nz, dtype):
    """``lds`` clipped to what ``_lds_planes`` accepts; None stays."""
    return lds and min(lds, nz, zline.MAX_LDS // (zline.BLOCK
                                                  * dtype.itemsize))


def check_solution(z, r, t, dtype, what, w=1):
    """``z`` against ``T^{-1} r`` on the interior at width ``w``, its halo
    zero; returns the error over ``eps kappa``."""
    nz = t.shape[0]
    ri = interior(r.cpu().double(), w)
    ref = torch.linalg.solve(
        t, ri.reshape(-1, nz, ri.shape[-2] * ri.shape[-1]))
    got = interior(z.cpu().double(), w).reshape(ref.shape)
    ratio = ((got - ref).abs().max() / ref.abs().max()
             / (torch.finfo(dtype).eps * kappa_inf(t))).item()
    assert ratio <= 16.0, (what, ratio)
    halo = z.clone()
    interior(halo, w).zero_()
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


def run_tall(grid, case, device, lds=None):
    """``solve`` of one row of ``TALL_CASES``; returns the ratio and the
    outputs."""
    zb, nz, w, dtype, bands, batch = case
    shape = (nz, 5 + 2 * w, 68 + 2 * w)
    nf = 1
    if batch:
        shape, nf = (batch,) + shape, 2
    t = dense_t(nz, *bands, zb)
    st = grid.make_stencil3d(shape, dtype, device, weights(*bands, w=w),
                             nfields=nf, z_boundary=zb)
    ls = st.make_line_solver(_lds_planes=clip_lds(lds, nz, dtype))
    assert ls.bands == bands and st.width == w
    g = torch.Generator().manual_seed(nz + w)
    r = [torch.randn(shape, generator=g, dtype=torch.float64).to(dtype)
         .to(device) for _ in range(nf)]
    keep = [f.clone() for f in r]
    z = as_tuple(ls.solve(*r))
    worst = 0.0
    for fz, fr, fk in zip(z, r, keep):
        assert torch.equal(fr, fk), "solve() mutated its input"
        worst = max(worst, check_solution(fz, fr, t, dtype, (case, lds), w))
    return worst, [f.cpu() for f in z]


def run_update(grid, zb, dtype, device, lds=None, shape=(2, 7, 41, 70), w=1):
    """One fused update against ``StencilCG.update_step`` and the dense
    solve, on integer data with ``alpha = 2``."""
    nf = 2
    st = grid.make_stencil3d(shape, dtype, device, weights(*BANDS, w=w),
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
    t = dense_t(shape[-3], *BANDS, zb)
    zs = as_tuple(pcg.preconditioned_residual)
    for fz, fr in zip(zs, pcg._r):
        check_solution(fz, fr, t, dtype, (zb, dtype, lds, shape), w)
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


def run_pcg(grids, name, device):
    """One row of ``PCG_CASES``: vertical weight 100, horizontal 1, the
    centre 1 above the sum of the others.  Accepted as the project's own
    solves are: ``converged``, and the true residual of the float64 oracle
    within ``10 rtol``.  Returns the iteration count."""
    dtype, zb, periodic, nf, shape, w, rtol = PCG_CASES[name]
    k = weights(-100.0, 201.0 + 4 * w, -100.0, h=-1.0, w=w)
    g = torch.Generator().manual_seed(11)
    b = [torch.nn.functional.pad(
        interior(torch.randn(shape, generator=g, dtype=torch.float64), w),
        (w,) * 4).to(dtype).to(device) for _ in range(nf)]
    st = grids[periodic].make_stencil3d(shape, dtype, device, k, nfields=nf,
                                        z_boundary=zb)
    x, info = st.make_cg("zline").solve(b if nf > 1 else b[0], rtol=rtol,
                                        maxiter=200, check_every=1)
    assert info.converged is True, (name, info)
    num = den = 0.0
    for fb, ax in zip(b, oracle(grids[periodic], k, as_tuple(x), zb)):
        bi = interior(fb.cpu().double(), w)
        num, den = num + (bi - ax).pow(2).sum(), den + bi.pow(2).sum()
    true = (num / den).sqrt().item()
    print("pcg", name, device, "iterations", info.iterations, "true", true)
    assert true <= 10 * rtol, (name, true)
    return info.iterations


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


@pytest.mark.parametrize("case", TALL_CASES, ids=case_id)
def test_tall_wide_line_solve_matches_dense(grids, case):
    print("err / (eps kappa):",
          run_tall(grids[(True, True)], case, "cpu")[0])


@pytest.mark.parametrize("zb", ZB)
@pytest.mark.parametrize("shape,w,dtype", UPDATE_CASES, ids=case_id)
def test_update_matches_composition_at_height(grids, shape, w, dtype, zb):
    run_update(grids[(True, True)], zb, dtype, "cpu", shape=shape, w=w)


@pytest.mark.parametrize("name", PCG_CASES)
def test_pcg_end_to_end(grids, name):
    run_pcg(grids, name, "cpu")


def test_singular_periodic_bands_are_refused(grids):
    """Periodic ``T`` with ``b = -(a + c)`` is singular at every height:
    the Sherman-Morrison denominator is 0 in real arithmetic, and between
    0 and eps in float64.  ``b`` larger by 1e-6 is accepted and solves to
    the dense reference within ``16 eps kappa`` (kappa is about 4e6)."""
    grid = grids[(True, True)]

    def make(nz, bands):
        return grid.make_stencil3d((nz, 3, 4), torch.float64, "cpu",
                                   weights(*bands), z_boundary="periodic")

    def accepts(st):
        try:
            st.make_line_solver()
        except ValueError as e:
            assert "not positive definite along z" in str(e)
            return False
        return True

    accepted = [(nz, bands) for nz in range(3, 71) for bands in SINGULAR
                if accepts(make(nz, bands))]
    assert not accepted, accepted
    for nz in range(3, 71):
        ls = make(nz, NEARLY).make_line_solver()
        assert torch.isfinite(ls.tables).all()
        if nz in (3, 33, 65):
            r = torch.randn(nz, 3, 4, dtype=torch.float64,
                            generator=torch.Generator().manual_seed(nz))
            ratio = check_solution(
                ls.solve(r), r, dense_t(nz, *NEARLY, "periodic"),
                torch.float64, ("nearly singular", nz))
            print("nz", nz, "err / (eps kappa):", ratio)


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
