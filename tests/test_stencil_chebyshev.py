"""CPU suite for parallel/chebyshev.StencilChebyshev
(``HaloStencil.make_chebyshev``) and ``HaloStencil.gershgorin_bounds``.

Exactness.  Two steps with dyadic coefficients on ``int_data`` and the
integer ``star`` weights stay exact in float32: with bounds (1, 3),
``theta = 2`` and ``d0 = r0 / 2`` is a half-integer below 2^7; after
``step(5/8, 3/4)`` and ``step(1/2, 1/2)`` every value and every partial
sum of a stencil is a multiple of 2^-5 below 2^18 at width 4 (row sums of
|weights| are at most 51), which fits 24 bits.  The oracle does the same
arithmetic in float64, where it is exact as well, and on shapes of up to
``RATIONAL_CELLS`` cells (all of the CPU suite's) again with
``fractions``, where results are compared as rationals; the GPU suite's
two large shapes are compared with the float64 oracle bitwise.

The SPD system, its right-hand side and ``true_residual`` are those of
tests/test_stencil_cg.py: ``A = I - 0.25 * lap``, eigenvalues in [1, 3]
at width 1 and in [1, 11/3] at width 2 (the fourth-order Laplacian's
symbol reaches -16/3 per axis), whatever the edges.

Bounds of the theorem.  With ``x0 = 0``, ``||r_k|| <= ||b|| / T_k(sigma)``
in exact arithmetic; rounding adds a term of the order of ``eps * k``,
which is why the theorem is only asserted while ``1 / T_k >= 50 * rtol``.
"""

import itertools
import math
from fractions import Fraction

import pytest
import torch
import torch.nn.functional as F

import mpi4jax_amd as m
from mpi4jax_amd.parallel import ChebyshevInfo, StencilChebyshev
from mpi4jax_amd.parallel.grid import CartesianGrid
from _mp import run_multiproc
from test_halo_adjoint import int_data
from test_halo_exchanger import DIMS, fake_grid
from test_halo_stencil import as_tuple, interior, make_weights, oracle_apply
from test_stencil_cg import (ALL_PERIODIC, GX, GY, LEVELS, SOLVES,
                             SPD_PERIODIC, frac, halo_of, spd_rhs,
                             spd_weights, true_residual)

STEPS = ((5 / 8, 3 / 4), (1 / 2, 1 / 2))
# (bounds, iterations_for at float64 1e-10, at float32 1e-5) by width;
# None stands for gershgorin_bounds()
TABLE = {1: [((1.0, 3.0), 19, 10)],
         2: [((1.0, 11 / 3), 21, 11), (None, 23, 12)]}
RATIONAL_CELLS = 2000  # fractions on shapes up to this many cells


def cheb_t(k, s):
    return math.cosh(k * math.acosh(s))


@pytest.fixture(scope="module")
def grids():
    m.init()
    return {p: CartesianGrid(dims=(1, 1), periodic=p) for p in ALL_PERIODIC}


# -------------------------------------------------------- two exact steps

def check_exact_steps(grid, shape, w, nf, dtype, device="cpu", **kw):
    """``start`` and the two ``STEPS`` with bounds (1, 3) against exact
    arithmetic; halos untouched; the direction buffers alternate.  Shared
    with the GPU suite."""
    k = make_weights("star", w, seed=2)
    st = grid.make_stencil(shape, dtype, device, k, nfields=nf, **kw)
    ch = st.make_chebyshev(1, 3)
    assert isinstance(ch, StencilChebyshev)
    assert (ch.theta, ch.delta, ch.sigma) == (2.0, 1.0, 2.0)
    b = [int_data(shape, dtype, 21 + i) for i in range(nf)]
    x = [torch.full(shape, 7.0, dtype=dtype) for _ in range(nf)]
    for t in x:
        interior(t, w).zero_()
    xd = [t.to(device) for t in x]
    ch.start([t.to(device) for t in b], xd)
    assert ch.iteration == 0
    rational = nf * b[0].numel() <= RATIONAL_CELLS

    # r0 = b - A x with the halo of x as boundary data; d0 = r0 / 2
    ax = oracle_apply(grid, k, x)
    xs = [torch.zeros_like(a) for a in ax]
    rs = [interior(t, w).double() - a for t, a in zip(b, ax)]
    ds = [r / 2 for r in rs]
    first = as_tuple(ch.direction)

    def compare(what, got, want):
        for g, e in zip(got, want):
            gi = interior(g, w).detach().cpu().double()  # exact
            if rational:
                assert frac(gi) == frac(e), (what, shape, w, dtype)
            else:
                assert torch.equal(gi, e), (what, shape, w, dtype)

    compare("r0", as_tuple(ch.residual), rs)
    compare("d0", first, ds)
    for n, (c1, c2) in enumerate(STEPS):
        qs = oracle_apply(grid, k, [F.pad(d, (w, w, w, w)) for d in ds])
        xn = [a + d for a, d in zip(xs, ds)]
        rn = [r - q for r, q in zip(rs, qs)]
        dn = [c1 * d + c2 * r for d, r in zip(ds, rn)]
        if rational:  # the float64 oracle is the rational one
            f1, f2 = Fraction(c1), Fraction(c2)
            for i in range(nf):
                fd, fq = frac(ds[i]), frac(qs[i])
                fr = [a - c for a, c in zip(frac(rs[i]), fq)]
                assert frac(xn[i]) == [a + c for a, c in
                                       zip(frac(xs[i]), fd)]
                assert frac(rn[i]) == fr
                assert frac(dn[i]) == [f1 * a + f2 * c
                                       for a, c in zip(fd, fr)]
        xs, rs, ds = xn, rn, dn
        before = as_tuple(ch.direction)
        ch.step(c1, c2)
        assert ch.iteration == n + 1
        after = as_tuple(ch.direction)
        for p, q in zip(before, after):
            assert p is not q, "d was updated in place"
        compare("x", xd, xs)
        compare("r", as_tuple(ch.residual), rs)
        compare("d", after, ds)
        for got in xd:
            assert torch.equal(halo_of(got, w), halo_of(x[0], w)), \
                "the halo of x was written"
        for got in as_tuple(ch.residual) + before + after:
            assert not halo_of(got, w).any(), "a halo of r or d was written"
    # two steps: back in the first buffer
    for p, q in zip(first, as_tuple(ch.direction)):
        assert p is q


@pytest.mark.parametrize("periodic", ALL_PERIODIC)
def test_two_steps_are_exact(grids, periodic):
    for (shape, w), nf, dtype in itertools.product(
            [((2, 9, 10), 1), ((2, 9, 10), 2), ((12, 13), 4)], (1, 3),
            (torch.float32, torch.float64)):
        check_exact_steps(grids[periodic], shape, w, nf, dtype)


# ------------------------------------------------- equality in the bound

@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_bound_is_attained_at_both_ends_of_the_spectrum(grids, dtype):
    """Fully periodic ``I - 0.25 * lap`` with bounds (1, 3): a constant is
    an eigenvector for 1 and ``(-1)^(i+j)`` on the 12 x 14 interior for 3,
    the two ends, where the residual polynomial equals ``1 / T_k(sigma)``
    and ``(-1)^k / T_k(sigma)``.  Tolerance ``450 * eps * max|b|``,
    absolute: about 40 roundings per step over 12 steps, derived and not
    measured."""
    grid, w = grids[(True, True)], 1
    st = grid.make_stencil((LEVELS, GY + 2, GX + 2), dtype, "cpu",
                           spd_weights(w))
    i = torch.arange(GY)[:, None] + torch.arange(GX)[None, :]
    alt = (1.0 - 2.0 * (i % 2)).expand(LEVELS, GY, GX)
    tol = 450 * torch.finfo(dtype).eps
    for bi, sign in ((torch.ones(LEVELS, GY, GX), 1.0), (alt, -1.0)):
        b = F.pad(bi, (w, w, w, w)).to(dtype)
        ch = st.make_chebyshev(1, 3)
        ch.start(b, torch.zeros_like(b))
        worst = 0.0
        for k in range(1, 13):
            ch.iterate(1)
            want = interior(b, w).double() * sign ** k / cheb_t(k, 2.0)
            err = (interior(ch.residual, w).double() - want).abs().max()
            worst = max(worst, err.item())
        print(dtype, sign, "worst", worst, "tol", tol)
        assert worst <= tol, (dtype, sign, worst)


# ------------------------------------------------------------------ solve

def table_cases(st, w):
    """``(bounds, (k at 1e-10, k at 1e-5))`` with Gershgorin's filled in."""
    for bounds, k64, k32 in TABLE[w]:
        if bounds is None:
            bounds = st.gershgorin_bounds()
            assert bounds == pytest.approx((5 / 6, 11 / 3), rel=1e-14)
        yield bounds, {1e-10: k64, 1e-5: k32}


def check_solve_table(grid, w, device="cpu"):
    """Shared with the GPU suite."""
    k = spd_weights(w)
    for dtype, rtol, _ in SOLVES:
        b = spd_rhs(w, dtype)
        bd = b.to(device)
        st = grid.make_stencil(b.shape, dtype, device, k)
        for bounds, counts in table_cases(st, w):
            ch = st.make_chebyshev(*bounds)
            n = ch.iterations_for(rtol)
            assert n == counts[rtol], (w, bounds, rtol, n)
            # a-priori count, no inner product
            x, info = ch.solve(bd, rtol=rtol, check_every=0)
            assert isinstance(info, ChebyshevInfo)
            assert info.iterations == n and info.converged is None
            assert isinstance(x, torch.Tensor) and x.device.type == device
            true = true_residual(grid, k, x, b)
            print(w, bounds, dtype, n, "true/rtol", true / rtol)
            assert true <= 2 * rtol, (w, bounds, dtype, true)
            assert not halo_of(x, w).any()
            # the theorem, one iteration at a time
            x = torch.zeros_like(bd)
            ch.start(bd, x)
            bnorm = interior(b, w).double().norm().item()
            worst, k_ = 0.0, 0
            while 1.0 / cheb_t(k_ + 1, ch.sigma) >= 50 * rtol:
                ch.iterate(1)
                k_ += 1
                rel = interior(ch.residual, w).double().norm().item() / bnorm
                worst = max(worst, rel * cheb_t(k_, ch.sigma))
            print(w, bounds, dtype, "max ||r_k|| T_k / ||b||", worst,
                  "over", k_, "iterations")
            assert k_ >= 5 and worst <= 1.0, (w, bounds, dtype, worst)
            # tested every iteration: converged within the a-priori count
            x, info = ch.solve(bd, rtol=rtol, check_every=1)
            assert info.converged is True and info.iterations <= n
            assert info.residual_norm <= rtol * info.rhs_norm
            assert info.rhs_norm == pytest.approx(bnorm, rel=1e-12)
            assert true_residual(grid, k, x, b) <= 2 * rtol


@pytest.mark.parametrize("periodic", SPD_PERIODIC)
@pytest.mark.parametrize("w", [1, 2])
def test_solve_table(grids, periodic, w):
    check_solve_table(grids[periodic], w)


def test_default_check_every_and_maxiter(grids):
    grid, w = grids[(True, False)], 2
    k = spd_weights(w)
    b = spd_rhs(w)
    st = grid.make_stencil(b.shape, torch.float64, "cpu", k, nfields=2)
    b2 = [b, b.flip(0).contiguous()]
    ch = st.make_chebyshev(1, 11 / 3)
    n = ch.iterations_for(1e-10)
    xa, ia = ch.solve(b2, rtol=1e-10)
    xb, ib = ch.solve(b2, rtol=1e-10)
    assert ia == ib and ia.converged
    assert ia.iterations in (n, 8 * math.ceil(
        ch.solve(b2, rtol=1e-10, check_every=1)[1].iterations / 8))
    for p, q in zip(xa, xb):
        assert torch.equal(p, q)
    _, short = ch.solve(b2, rtol=1e-10, maxiter=3)
    assert short.iterations == 3 and short.converged is False
    _, loose = ch.solve(b2, rtol=0.0, atol=1e-3 * ia.rhs_norm,
                        maxiter=40, check_every=1)
    assert loose.converged and loose.iterations < ia.iterations


@pytest.mark.parametrize("w", [1, 2])
def test_closed_edges_hold_dirichlet_data(grids, w):
    bounds = TABLE[w][0][0]
    for periodic, (dtype, rtol, _) in itertools.product(
            [(False, False), (True, False)], SOLVES):
        grid = grids[periodic]
        k = spd_weights(w)
        b = spd_rhs(w, dtype)
        g = torch.Generator().manual_seed(8)
        x0 = torch.randn(b.shape, generator=g).to(dtype)
        keep = x0.clone()
        st = grid.make_stencil(b.shape, dtype, "cpu", k)
        # r0 is not b here: test the residual instead of counting a priori
        x, info = st.make_chebyshev(*bounds).solve(
            b, x0, rtol=rtol, maxiter=40, check_every=1)
        assert info.converged
        assert torch.equal(x0, keep), "solve wrote x0"
        assert torch.equal(halo_of(x, w), halo_of(x0, w)), "halo changed"
        assert true_residual(grid, k, x, b) <= 2 * rtol


def test_non_finite_residual_raises(grids):
    st = grids[(True, True)].make_stencil((9, 10), torch.float32, "cpu",
                                          spd_weights(1))
    b = torch.ones(9, 10)
    b[4, 4] = float("inf")
    with pytest.raises(FloatingPointError):
        st.make_chebyshev(1, 3).solve(b, maxiter=4)
    # bounds that exclude an eigenvalue: the iteration diverges, and a
    # test notices once the residual overflows
    b = spd_rhs(1, torch.float32)
    st = grids[(True, True)].make_stencil(b.shape, torch.float32, "cpu",
                                          spd_weights(1))
    with pytest.raises(FloatingPointError):
        st.make_chebyshev(1, 1.5).solve(b, maxiter=400, check_every=50)


# ------------------------------------------- decomposition invariance

def _multirank(rank, ws):
    comm = m.get_world()
    dims_list = [d for d in DIMS[ws] if GY % d[0] == 0 and GX % d[1] == 0]
    assert len(dims_list) >= 2
    for dims, periodic, w in itertools.product(dims_list, SPD_PERIODIC,
                                               (1, 2)):
        grid = CartesianGrid(comm=comm, dims=dims, periodic=periodic)
        one = fake_grid(0, (1, 1), periodic)
        by, bx = GY // dims[0], GX // dims[1]
        cy, cx = grid.coords

        def block(t):
            return F.pad(
                interior(t, w)[..., cy * by:(cy + 1) * by,
                               cx * bx:(cx + 1) * bx],
                (w, w, w, w)).contiguous()

        k = spd_weights(w)
        bounds = TABLE[w][0][0]
        for dtype in (torch.float64, torch.float32):
            B = spd_rhs(w, dtype)
            X = torch.zeros_like(B)
            ch1 = one.make_stencil(B.shape, dtype, "cpu",
                                   k).make_chebyshev(*bounds)
            ch1.start(B, X)
            ch1.iterate(10)
            b = block(B)
            x = torch.zeros_like(b)
            ch = grid.make_stencil(b.shape, dtype, "cpu",
                                   k).make_chebyshev(*bounds)
            ch.start(b, x)
            ch.iterate(10)
            assert ch.iteration == 10
            what = (dims, periodic, w, dtype)
            assert torch.equal(interior(x, w), interior(block(X), w)), what
            assert torch.equal(interior(ch.residual, w),
                               interior(block(ch1.residual), w)), what
            assert interior(x, w).abs().max() > 0


@pytest.mark.parametrize("ws", [2, 4])
def test_decomposed_run_equals_single_domain_bitwise(ws):
    """One spawn per world size.  No reductions: every rank's interior of
    ``x`` and ``r`` after 10 iterations is bitwise the world-1 result."""
    run_multiproc(_multirank, ws)


# ------------------------------------------------------------- validation

def test_coefficients_and_iterations_for(grids):
    st = grids[(True, True)].make_stencil((9, 10), torch.float64, "cpu",
                                          spd_weights(1))
    ch = st.make_chebyshev(1, 3)
    # sigma = 2, delta = 1: rho = 1/2, 2/7, 7/26, 26/97 = T_k / T_{k+1}
    rho = [1 / 2, 2 / 7, 7 / 26, 26 / 97]
    for k in (2, 0, 1):
        c1, c2 = ch.coefficients(k)
        assert isinstance(c1, float) and isinstance(c2, float)
        assert c1 == pytest.approx(rho[k + 1] * rho[k], rel=1e-15)
        assert c2 == pytest.approx(2 * rho[k + 1], rel=1e-15)
    for k in (-1, 1.0, True):
        with pytest.raises(ValueError, match="non-negative"):
            ch.coefficients(k)
    # 1 / T_k(2) = 1, 1/2, 1/7, 1/26, 1/97
    assert ch.iterations_for(1.0) == 0 and ch.iterations_for(0.6) == 1
    assert ch.iterations_for(0.2) == 2 and ch.iterations_for(0.1) == 3
    assert ch.iterations_for(0.03) == 4 and ch.iterations_for(7.0) == 0
    with pytest.raises(ValueError, match="positive"):
        ch.iterations_for(0.0)
    assert st.gershgorin_bounds() == (1.0, 3.0)
    lo, hi = grids[(True, True)].make_stencil(
        (9, 10), torch.float32, "cpu",
        make_weights("asym", 1)).gershgorin_bounds()
    kk = make_weights("asym", 1)
    off = kk.abs().sum().item() - abs(kk[1, 1].item())
    assert (lo, hi) == (kk[1, 1].item() - off, kk[1, 1].item() + off)


def test_validation(grids):
    grid = grids[(True, True)]
    k = spd_weights(1)
    for dtype in (torch.bfloat16, torch.float16):
        with pytest.raises(TypeError, match="float32 and float64"):
            grid.make_stencil((9, 10), dtype, "cpu", k).make_chebyshev(1, 3)
    st = grid.make_stencil((2, 9, 10), torch.float32, "cpu", k, nfields=2)
    for bounds in ((0.0, 3.0), (-1.0, 3.0), (3.0, 3.0), (3.0, 1.0),
                   (1.0, math.inf), (math.nan, 3.0), (1.0, math.nan)):
        with pytest.raises(ValueError, match="0 < lmin < lmax < inf"):
            st.make_chebyshev(*bounds)
    with pytest.raises(TypeError, match="real number"):
        st.make_chebyshev("1", 3)
    ch = st.make_chebyshev(1, 3)
    a = torch.ones(2, 9, 10)
    b = torch.ones(2, 9, 10)
    for fn in (ch.iterate, lambda: ch.step(0.5, 0.5)):
        with pytest.raises(RuntimeError, match="start"):
            fn()
    bad = [((a,), ValueError, "2 field"),
           ((a, torch.ones(2, 9, 11)), ValueError, "shape"),
           ((a, b.double()), TypeError, "dtype"),
           ((a, torch.ones(2, 9, 20)[..., ::2]), ValueError, "contiguous")]
    for fields, exc, match in bad:
        with pytest.raises(exc, match=match):
            ch.start((a, b), fields)
        with pytest.raises(exc, match=match):
            ch.start(fields, (a, b))
        with pytest.raises(exc, match=match):
            ch.solve(fields)
        with pytest.raises(exc, match=match):
            ch.solve((a, b), fields)
    big = torch.ones(3, 2, 9, 10)
    with pytest.raises(ValueError, match="overlaps"):
        ch.start((a, b), (a, big[0]))  # x overlapping b
    with pytest.raises(ValueError, match="overlaps"):
        ch.start((a, b), (big[0], big[0]))
    for kw in (dict(maxiter=0), dict(maxiter=-1), dict(check_every=-1)):
        with pytest.raises(ValueError, match="maxiter|check_every"):
            ch.solve((a, b), **kw)
    for kw in (dict(maxiter=2.5), dict(check_every=1.0),
               dict(maxiter=True), dict(check_every=None)):
        with pytest.raises(TypeError, match="int"):
            ch.solve((a, b), **kw)
    with pytest.raises(ValueError, match="non-negative"):
        ch.iterate(-1)
    # nothing above touched a buffer or started a solve
    assert torch.equal(a, torch.ones(2, 9, 10)) and bool((big == 1).all())
    for t in as_tuple(ch.residual) + as_tuple(ch.direction):
        assert not t.any()
    with pytest.raises(RuntimeError, match="start"):
        ch.iterate()
    ch.start((a, b), (torch.zeros(2, 9, 10), torch.zeros(2, 9, 10)))
    for c in (math.inf, math.nan):
        with pytest.raises(ValueError, match="finite"):
            ch.step(c, 0.5)
        with pytest.raises(ValueError, match="finite"):
            ch.step(0.5, c)
    assert ch.iteration == 0
    # check_every=0: device tensors, nothing reduced, nothing judged
    x, info = ch.solve((a, b), rtol=1e-3, check_every=0)
    assert info == ChebyshevInfo(ch.iterations_for(1e-3), None, None, None)
    assert isinstance(x, tuple) and len(x) == 2
    assert all(isinstance(t, torch.Tensor) and t.device == a.device
               for t in x)
