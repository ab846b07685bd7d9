"""CPU suite for the Krylov layer over parallel/stencil.HaloStencil:
``dot``, ``apply_dot`` and parallel/cg.StencilCG (``make_cg``).

Exactness.  On ``int_data`` (integers in [-4, 4]) with the integer weights
of ``make_weights`` every product and every partial sum of an inner
product is an integer far below 2^53, so ``dot`` and ``apply_dot`` are
compared with integer arithmetic on ``oracle_apply``'s result, for any
order of additions.  One CG iteration with dyadic ``alpha`` and
``beta`` is exact in float32 as well and is compared with ``fractions``.

The SPD test system.  ``A = I - 0.25 * lap`` with the 5-point Laplacian
(width 1) or the fourth-order one of examples/fused_stencil_diffusion.py
(width 2) on a 12 x 14 interior, 2 levels, ``b = randn`` with seed 3.  Its
eigenvalues are 1 - 0.25 * (those of lap) >= 1 whatever the edges (closed
edges with a zero halo are Dirichlet conditions, and lap is negative
semi-definite under both), so ``lambda_min(A) >= 1`` and
``|x - y| <= |A x - A y|``.

Expected iteration counts, with float64 inner products and a test after
every iteration: float64 at rtol 1e-10 stops after 18 (width 1) and 20
(width 2) iterations; float32 at rtol 1e-5 after 9 and 10 or 11 (11 at
width 2 with a periodic axis).  The true relative residual, ``A`` applied
in float64, is between 0.30 and 0.92 of rtol and within 0.2 % of the
recurrence residual.  The caps are about twice those counts, 40 and 20;
the true residual must be <= 2 * rtol.
"""

import itertools
import math
from fractions import Fraction

import pytest
import torch
import torch.nn.functional as F

import mpi4jax_amd as m
from mpi4jax_amd.parallel import CGInfo, StencilCG
from mpi4jax_amd.parallel.grid import CartesianGrid
from _mp import run_multiproc
from test_halo_adjoint import int_data
from test_halo_exchanger import DIMS, fake_grid
from test_halo_stencil import as_tuple, interior, make_weights, oracle_apply

DTYPES = (torch.float64, torch.float32, torch.bfloat16, torch.float16)
SPD_PERIODIC = [(True, True), (True, False), (False, False)]
ALL_PERIODIC = SPD_PERIODIC + [(False, True)]
# (dtype, rtol, iteration cap) of the module docstring's table
SOLVES = [(torch.float64, 1e-10, 40), (torch.float32, 1e-5, 20)]
GY, GX, LEVELS = 12, 14, 2  # the SPD system's interior


# ---------------------------------------------------------------- helpers

def spd_weights(w):
    """``I - 0.25 * lap`` as a (2w+1, 2w+1) float64 table, w in (1, 2)."""
    n = 2 * w + 1
    axis = {1: [1.0, -2.0, 1.0],
            2: [x / 12.0 for x in (-1.0, 16.0, -30.0, 16.0, -1.0)]}[w]
    axis = torch.tensor(axis, dtype=torch.float64)
    k = torch.zeros(n, n, dtype=torch.float64)
    k[w, :] -= 0.25 * axis
    k[:, w] -= 0.25 * axis
    k[w, w] += 1.0
    return k


def spd_rhs(w, dtype=torch.float64):
    """The global right-hand side, zero halo of width w."""
    g = torch.Generator().manual_seed(3)
    b = torch.randn(LEVELS, GY, GX, generator=g, dtype=torch.float64)
    return F.pad(b, (w, w, w, w)).to(dtype)


def true_residual(grid, k, x, b):
    """``||b - A x|| / ||b||`` over the interior, ``A`` applied in float64
    by the oracle (one field)."""
    w = (k.shape[0] - 1) // 2
    (ax,) = oracle_apply(grid, k, [x.detach().cpu().double()])
    bi = interior(b.detach().cpu().double(), w)
    return ((bi - ax).norm() / bi.norm()).item()


def int_dot(a, b):
    """Integer inner product of two integer-valued tensors: int64
    arithmetic (no rounding anywhere), returned as a Python int."""
    fa = a.detach().cpu().double()
    fb = b.detach().cpu().double()
    ia, ib = fa.to(torch.int64), fb.to(torch.int64)
    assert torch.equal(ia.double(), fa) and torch.equal(ib.double(), fb)
    return int((ia * ib).sum().item())


def frac(t):
    return [Fraction(v) for v in t.detach().cpu().double().reshape(-1).tolist()]


def halo_of(t, w, fill=0.0):
    """``t`` with its interior overwritten by ``fill``."""
    h = t.detach().cpu().clone()
    interior(h, w).fill_(fill)
    return h


@pytest.fixture(scope="module")
def grids():
    m.init()
    return {p: CartesianGrid(dims=(1, 1), periodic=p) for p in ALL_PERIODIC}


def check_exact_dots(grid, shape, w, nf, dtype, device="cpu", **kw):
    """dot / apply_dot on int_data against integer arithmetic.  Shared
    with the GPU suite, which goes on with what this returns: the stencil,
    its two field lists, apply's outputs and the two expected values."""
    k = make_weights("asym", w, seed=nf)
    base = [int_data(shape, torch.float64, 11 * i + nf) for i in range(nf)]
    other = [int_data(shape, torch.float64, 13 * i + nf + 5)
             for i in range(nf)]
    exp = [e.to(dtype).double() for e in oracle_apply(grid, k, base)]
    st = grid.make_stencil(shape, dtype, device, k, nfields=nf, **kw)
    x = [t.to(dtype).to(device) for t in base]
    y = [t.to(dtype).to(device) for t in other]
    want_xy = sum(int_dot(interior(a, w), interior(c, w))
                  for a, c in zip(base, other))
    want_xx = sum(int_dot(interior(a, w), interior(a, w)) for a in base)
    want_pap = sum(int_dot(interior(a, w), e) for a, e in zip(base, exp))
    arg = (lambda ts: ts[0]) if nf == 1 else (lambda ts: ts)
    d = st.dot(arg(x), arg(y))
    assert d.dtype == torch.float64 and d.dim() == 0
    assert d.device.type == device
    assert d.item() == want_xy, (shape, w, nf, dtype)
    assert st.dot(arg(x), arg(x)).item() == want_xx, (shape, w, nf, dtype)
    ref = as_tuple(st.apply(*x))
    out, pap = st.apply_dot(*x)
    assert isinstance(out, tuple) == (nf > 1)
    for o, r in zip(as_tuple(out), ref):
        assert torch.equal(o, r), "apply_dot's out differs from apply's"
    assert pap.dtype == torch.float64 and pap.dim() == 0
    assert pap.item() == want_pap, (shape, w, nf, dtype)
    # out= form: halos kept, same numbers
    outs = [torch.full(shape, 7.0, dtype=dtype, device=device)
            for _ in range(nf)]
    got, pap2 = st.apply_dot(*x, out=arg(outs))
    assert pap2.item() == want_pap
    for g, o, r in zip(as_tuple(got), outs, ref):
        assert g is o
        assert torch.equal(interior(o, w), interior(r, w))
        assert torch.equal(halo_of(o, w, 7.0),
                           torch.full(shape, 7.0, dtype=dtype))
    for t, keep in zip(x + y, base + other):
        assert torch.equal(t.cpu().double(), keep), "an input was written"
    return st, x, y, ref, want_xy, want_pap


# ------------------------------------------------------------ exact dots

@pytest.mark.parametrize("periodic", ALL_PERIODIC)
@pytest.mark.parametrize("w", [1, 2, 3, 4])
def test_dot_and_apply_dot_are_exact(grids, periodic, w):
    shapes = [(3 * w, 3 * w + 1), (2, 12, 13), (2, 3, 13, 12)]
    for shape, nf, dtype in itertools.product(shapes, (1, 3), DTYPES):
        check_exact_dots(grids[periodic], shape, w, nf, dtype)


# --------------------------------------------------- one exact iteration

def check_exact_iteration(grid, shape, w, nf, dtype, device="cpu", **kw):
    """One update and one direction step with alpha = 3/4 and beta = 5/8
    against ``fractions``; halos untouched.  Shared with the GPU suite."""
    k = make_weights("star", w, seed=2)
    st = grid.make_stencil(shape, dtype, device, k, nfields=nf, **kw)
    cg = st.make_cg()
    assert isinstance(cg, StencilCG)
    b = [int_data(shape, dtype, 21 + i) for i in range(nf)]
    x = [torch.full(shape, 7.0, dtype=dtype) for _ in range(nf)]
    for t in x:
        interior(t, w).zero_()
    xd = [t.to(device) for t in x]
    cg.start([t.to(device) for t in b], xd)
    # r0 = b - A x with the halo of x as boundary data
    ax = oracle_apply(grid, k, x)
    r0 = [interior(t, w).double() - a for t, a in zip(b, ax)]
    rs0 = sum(int_dot(r, r) for r in r0)
    assert cg.rs.item() == rs0
    for r, p, e in zip(as_tuple(cg.residual), as_tuple(cg.direction), r0):
        assert torch.equal(interior(r.cpu(), w).double(), e)
        assert torch.equal(p, r)
    cg.apply_step()
    p0 = [F.pad(r, (w, w, w, w)) for r in r0]
    q0 = oracle_apply(grid, k, p0)
    assert cg.pq.item() == sum(int_dot(r, q) for r, q in zip(r0, q0))

    cg.rs.fill_(3.0)
    cg.pq.fill_(4.0)
    cg.update_step()
    alpha = Fraction(3, 4)
    want_x = [[alpha * v for v in frac(r)] for r in r0]
    want_r = [[a - alpha * c for a, c in zip(frac(r), frac(q))]
              for r, q in zip(r0, q0)]
    want_rs = sum(v * v for f in want_r for v in f)
    assert Fraction(cg.rs.item()) == want_rs
    assert cg.rs_old.item() == 3.0
    for got, want in zip(xd, want_x):
        assert frac(interior(got, w)) == want
        assert torch.equal(halo_of(got, w), halo_of(x[0], w)), \
            "the halo of x was written"
    for got, want in zip(as_tuple(cg.residual), want_r):
        assert frac(interior(got, w)) == want
        assert not halo_of(got, w).any(), "the halo of r was written"

    cg.rs.fill_(5.0)
    cg.rs_old.fill_(8.0)
    cg.direction_step()
    beta = Fraction(5, 8)
    for got, rn, pold in zip(as_tuple(cg.direction), want_r, r0):
        want = [a + beta * c for a, c in zip(rn, frac(pold))]
        assert frac(interior(got, w)) == want
        assert not halo_of(got, w).any(), "the halo of p was written"
    assert cg.rs.item() == 5.0 and cg.rs_old.item() == 8.0


@pytest.mark.parametrize("periodic", ALL_PERIODIC)
def test_one_iteration_is_exact(grids, periodic):
    for (shape, w), nf, dtype in itertools.product(
            [((2, 9, 10), 1), ((2, 9, 10), 2), ((12, 13), 4)], (1, 3),
            (torch.float32, torch.float64)):
        check_exact_iteration(grids[periodic], shape, w, nf, dtype)


# ------------------------------------------------------------------ solve

@pytest.mark.parametrize("periodic", SPD_PERIODIC)
@pytest.mark.parametrize("w", [1, 2])
def test_solve_table(grids, periodic, w):
    grid = grids[periodic]
    k = spd_weights(w)
    for dtype, rtol, cap in SOLVES:
        b = spd_rhs(w, dtype)
        st = grid.make_stencil(b.shape, dtype, "cpu", k)
        keep = b.clone()
        x, info = st.make_cg().solve(b, rtol=rtol, maxiter=cap,
                                     check_every=1)
        assert isinstance(info, CGInfo) and info.converged is True
        assert info.iterations <= cap
        assert info.residual_norm <= rtol * info.rhs_norm
        assert info.rhs_norm == pytest.approx(
            interior(b, w).double().norm().item(), rel=1e-12)
        true = true_residual(grid, k, x, b)
        print(periodic, w, dtype, info.iterations, true / rtol,
              info.residual_norm / info.rhs_norm / rtol)
        assert true <= 2 * rtol, (periodic, w, dtype, true)
        assert torch.equal(b, keep) and not halo_of(x, w).any()
        # the default check_every tests every 8th iteration
        x8, info8 = st.make_cg().solve(b, rtol=rtol, maxiter=cap)
        assert info8.converged and info8.iterations <= cap
        assert info8.iterations in (
            cap, 8 * math.ceil(info.iterations / 8))
        assert true_residual(grid, k, x8, b) <= 2 * rtol
        # check_every=0: exactly maxiter iterations, nothing read back
        x0, info0 = st.make_cg().solve(b, rtol=rtol, maxiter=cap,
                                       check_every=0)
        assert info0.iterations == cap and info0.converged is None
        assert isinstance(info0.residual_norm, torch.Tensor)
        assert true_residual(grid, k, x0, b) <= 2 * rtol


def test_two_solves_agree_bitwise_and_maxiter_is_honoured(grids):
    grid, w = grids[(True, False)], 2
    k = spd_weights(w)
    b = spd_rhs(w)
    st = grid.make_stencil(b.shape, torch.float64, "cpu", k, nfields=2)
    b2 = [b, b.flip(0).contiguous()]
    cg = st.make_cg()
    xa, ia = cg.solve(b2, rtol=1e-10, maxiter=40)
    xb, ib = cg.solve(b2, rtol=1e-10, maxiter=40)
    assert ia == ib and ia.converged
    for p, q in zip(xa, xb):
        assert torch.equal(p, q)
    _, short = cg.solve(b2, rtol=1e-10, maxiter=3)
    assert short.iterations == 3 and short.converged is False
    # atol alone
    _, loose = cg.solve(b2, rtol=0.0, atol=1e-3 * ia.rhs_norm, maxiter=40,
                        check_every=1)
    assert loose.converged and loose.iterations < ia.iterations


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
        for dtype, rtol, cap in SOLVES:
            B = spd_rhs(w, dtype)
            st1 = one.make_stencil(B.shape, dtype, "cpu", k)
            X, _ = st1.make_cg().solve(B, rtol=rtol, maxiter=cap,
                                       check_every=1)
            b = block(B)
            st = grid.make_stencil(b.shape, dtype, "cpu", k)
            x, info = st.make_cg().solve(b, rtol=rtol, maxiter=cap,
                                         check_every=1)
            assert info.converged and info.iterations <= cap
            diff = (interior(x, w).double()
                    - interior(block(X), w).double())
            err = math.sqrt(m.allreduce((diff * diff).sum(), m.SUM,
                                        comm=comm).item())
            bnorm = interior(B, w).double().norm().item()
            assert info.rhs_norm == pytest.approx(bnorm, rel=1e-12)
            assert err <= 4 * rtol * bnorm, (dims, periodic, w, dtype, err)
        if ws == 2:
            # decomposed dot == single-domain dot, exactly, on integers
            kk = make_weights("asym", w, seed=1)
            G = [F.pad(int_data((3, GY, GX), torch.float64, 60 + i),
                       (w, w, w, w)) for i in range(2)]
            H = [F.pad(int_data((3, GY, GX), torch.float64, 70 + i),
                       (w, w, w, w)) for i in range(2)]
            st1 = one.make_stencil(G[0].shape, torch.float64, "cpu", kk,
                                   nfields=2)
            g, h = [block(t) for t in G], [block(t) for t in H]
            st = grid.make_stencil(g[0].shape, torch.float64, "cpu", kk,
                                   nfields=2)
            want = sum(int_dot(interior(a, w), interior(c, w))
                       for a, c in zip(G, H))
            assert st.dot(g, h).item() == want == st1.dot(G, H).item()
            assert st.apply_dot(*g)[1].item() == st1.apply_dot(*G)[1].item()


@pytest.mark.parametrize("ws", [2, 4])
def test_multirank_solve_equals_single_domain(ws):
    """One spawn per world size.  Both solutions have a true residual
    <= 2 * rtol * ||b|| and lambda_min(A) >= 1, so they differ by at most
    4 * rtol * ||b|| in the 2-norm."""
    run_multiproc(_multirank, ws)


# --------------------------------------------------------- Dirichlet data

@pytest.mark.parametrize("w", [1, 2])
def test_closed_edges_hold_dirichlet_data(grids, w):
    for periodic, (dtype, rtol, cap) in itertools.product(
            [(False, False), (True, False)], SOLVES):
        grid = grids[periodic]
        k = spd_weights(w)
        b = spd_rhs(w, dtype)
        g = torch.Generator().manual_seed(8)
        x0 = torch.randn(b.shape, generator=g).to(dtype)
        keep = x0.clone()
        st = grid.make_stencil(b.shape, dtype, "cpu", k)
        x, info = st.make_cg().solve(b, x0, rtol=rtol, maxiter=cap,
                                     check_every=1)
        assert info.converged
        assert torch.equal(x0, keep), "solve wrote x0"
        assert torch.equal(halo_of(x, w), halo_of(x0, w)), "halo changed"
        # A x = b with that halo: the oracle reads the halo of x
        assert true_residual(grid, k, x, b) <= 2 * rtol
        # and the data matters: the zero-halo solution differs
        z, _ = st.make_cg().solve(b, rtol=rtol, maxiter=cap, check_every=1)
        assert (interior(z, w) - interior(x, w)).abs().max() > 1e-3


# ------------------------------------------------------ degenerate cases

def test_degenerate_cases_stay_finite(grids):
    for periodic, dtype in itertools.product(SPD_PERIODIC,
                                             (torch.float32, torch.float64)):
        grid = grids[periodic]
        shape, w = (2, 9, 10), 1
        st = grid.make_stencil(shape, dtype, "cpu", spd_weights(w))
        cg = st.make_cg()
        x = torch.zeros(shape, dtype=dtype)
        cg.start(torch.zeros(shape, dtype=dtype), x)
        cg.iterate(5)
        assert cg.rs.item() == 0.0 and not x.any()
        assert not torch.isnan(cg.direction).any()
        # 2 * I: one iteration is the solve, five more change nothing
        two = torch.zeros(3, 3, dtype=torch.float64)
        two[1, 1] = 2.0
        st = grid.make_stencil(shape, dtype, "cpu", two)
        cg = st.make_cg()
        b = int_data(shape, dtype, 4)
        x = torch.zeros(shape, dtype=dtype)
        cg.start(b, x)
        cg.iterate(1)
        assert torch.equal(interior(x, w), interior(b, w) / 2)
        assert cg.rs.item() == 0.0
        keep = x.clone()
        cg.iterate(5)
        assert torch.equal(x, keep) and cg.rs.item() == 0.0
        for t in (cg.direction, cg.residual):
            assert torch.isfinite(t).all()
        _, info = cg.solve(b, rtol=1e-6, maxiter=10, check_every=1)
        assert info.iterations == 1 and info.converged


def test_non_finite_rs_raises(grids):
    st = grids[(True, True)].make_stencil((9, 10), torch.float32, "cpu",
                                          spd_weights(1))
    b = torch.ones(9, 10)
    b[4, 4] = float("inf")
    with pytest.raises(FloatingPointError):
        st.make_cg().solve(b, maxiter=4)


# ------------------------------------------------------------- validation

def test_validation(grids):
    grid = grids[(True, True)]
    k = spd_weights(1)
    for dtype in (torch.bfloat16, torch.float16):
        with pytest.raises(TypeError, match="float32 and float64"):
            grid.make_stencil((9, 10), dtype, "cpu", k).make_cg()
    st = grid.make_stencil((2, 9, 10), torch.float32, "cpu", k, nfields=2)
    cg = st.make_cg()
    a = torch.ones(2, 9, 10)
    b = torch.ones(2, 9, 10)
    for fn in (cg.iterate, cg.apply_step, cg.update_step,
               cg.direction_step):
        with pytest.raises(RuntimeError, match="start"):
            fn()
    bad = [((a,), ValueError, "2 field"),
           ((a, b, a), ValueError, "2 field"),
           ((a, torch.ones(2, 9, 11)), ValueError, "shape"),
           ((a, b.double()), TypeError, "dtype"),
           ((a, torch.ones(2, 9, 20)[..., ::2]), ValueError, "contiguous"),
           ((a, torch.ones(2, 9, 10, device="meta")), ValueError, "lives on")]
    for fields, exc, match in bad:
        with pytest.raises(exc, match=match):
            st.dot(fields, (a, b))
        with pytest.raises(exc, match=match):
            st.dot((a, b), fields)
        with pytest.raises(exc, match=match):
            st.apply_dot(*fields)
        with pytest.raises(exc, match=match):
            cg.start((a, b), fields)
        with pytest.raises(exc, match=match):
            cg.start(fields, (a, b))
        with pytest.raises(exc, match=match):
            cg.solve(fields, maxiter=3)
        with pytest.raises(exc, match=match):
            cg.solve((a, b), fields, maxiter=3)
    big = torch.ones(3, 2, 9, 10)
    with pytest.raises(ValueError, match="overlaps input"):
        st.apply_dot(a, b, out=(a, torch.zeros(2, 9, 10)))
    with pytest.raises(ValueError, match="overlaps out"):
        st.apply_dot(a, b, out=(big[0], big[0]))
    with pytest.raises(ValueError, match="overlaps"):
        cg.start((a, b), (a, big[0]))
    with pytest.raises(ValueError, match="overlaps"):
        cg.start((a, b), (big[0], big[0]))
    for kw in (dict(maxiter=0), dict(maxiter=-1),
               dict(maxiter=3, check_every=-1)):
        with pytest.raises(ValueError, match="maxiter|check_every"):
            cg.solve((a, b), **kw)
    with pytest.raises(TypeError):
        cg.solve((a, b))  # maxiter is required
    with pytest.raises(TypeError, match="int"):
        cg.solve((a, b), maxiter=2.5)
    with pytest.raises(ValueError, match="non-negative"):
        cg.iterate(-1)
    # nothing above touched a buffer
    assert torch.equal(a, torch.ones(2, 9, 10)) and bool((big == 1).all())
    assert torch.equal(b, torch.ones(2, 9, 10))
    for t in as_tuple(cg.residual) + as_tuple(cg.direction):
        assert not t.any()
    with pytest.raises(RuntimeError, match="start"):
        cg.iterate()
