"""CPU suite for parallel/stencil.HaloStencil (``CartesianGrid.make_stencil``):
``apply``, ``adjoint`` and the differentiable ``apply_ad``.

Reference for values: ``HaloExchanger.exchange`` on a float64 copy, then
the tap sum in float64 by explicit slicing written here (``oracle_apply``).
Reference for the adjoint: ``S^T`` by ``index_add_`` over the same taps,
then ``E^T`` by ``oracle_adjoint`` over ``source_map`` of
tests/test_halo_adjoint.py (``oracle_adjoint_chain``).

Exactness.  Integer data in [-4, 4] with integer weights in [-3, 3] makes
every partial sum exact in float32 and float64 (at most 81*4*3 = 972), so
results are compared bitwise; float16 / bfloat16 after the single
round-to-nearest-even, which the oracle applies where the library does.

Random data is held to the a-priori bound
``|got - exact| <= gamma(n + 2) * sum_t |K_t| |x_t| + u_out * |exact|``
with ``gamma(k) = k u / (1 - k u)``, ``n`` the number of taps, ``u`` the
unit roundoff of the accumulate type and ``u_out`` that of a float16 /
bfloat16 store.  It holds for any order of adds, fused or not.
"""

import itertools
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import mpi4jax_amd as m
from mpi4jax_amd.parallel import HaloStencil
from mpi4jax_amd.parallel.grid import CartesianGrid
from _mp import run_multiproc
from test_halo_exchanger import DIMS, ENV, PERIODIC, REPO, fake_grid
from test_halo_adjoint import int_data, oracle_adjoint, source_map

DTYPES = (torch.float64, torch.float32, torch.bfloat16, torch.float16)


# ---------------------------------------------------------------- helpers

def as_tuple(out):
    return out if isinstance(out, tuple) else (out,)


def fits(shape, w):
    return shape[-2] >= 3 * w and shape[-1] >= 3 * w


def make_weights(kind, r, seed=0):
    """Integer weights in [-3, 3] as a (2r+1, 2r+1) float64 tensor."""
    n = 2 * r + 1
    g = torch.Generator().manual_seed(100 * r + seed)
    k = torch.zeros(n, n, dtype=torch.float64)
    if kind == "full":  # every tap present
        k = torch.randint(1, 4, (n, n), generator=g).double()
        k *= torch.randint(0, 2, (n, n), generator=g).double() * 2 - 1
    elif kind == "star":  # the two axes through the centre
        k[r, :] = torch.randint(1, 4, (n,), generator=g).double()
        k[:, r] = -torch.randint(1, 4, (n,), generator=g).double()
        k[r, r] = 3.0
    elif kind == "single":  # one tap, off-centre, at the far corner
        k[2 * r, 0] = -2.0
    elif kind == "asym":  # zeros mixed in, no symmetry
        k = torch.randint(-3, 4, (n, n), generator=g).double()
        k[0, n - 1] = 3.0
        k[n - 1, 0] = 0.0
    else:
        raise ValueError(kind)
    return k


KINDS = ("full", "star", "single", "asym")


def unit_acc(dtype):
    return 2.0 ** -53 if dtype == torch.float64 else 2.0 ** -24


def unit_out(dtype):
    return {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}.get(
        dtype, 0.0)


def gamma(k, u):
    return k * u / (1.0 - k * u)


def ntaps(weights):
    return int((torch.as_tensor(weights) != 0).sum())


def oracle_apply(grid, weights, fields, with_mag=False):
    """Interior of ``A`` on ``fields`` in float64: list of
    (levels..., ny - 2w, nx - 2w) tensors; with ``with_mag`` also
    ``sum_t |K_t| |x_t|``."""
    k = torch.as_tensor(weights, dtype=torch.float64)
    w = (k.shape[0] - 1) // 2
    shape = tuple(fields[0].shape)
    ny, nx = shape[-2:]
    ex = grid.make_halo_exchanger(shape, torch.float64, "cpu", width=w,
                                  nfields=len(fields))
    vs = as_tuple(ex.exchange(*(f.detach().cpu().double() for f in fields)))
    outs, mags = [], []
    for v in vs:
        o = torch.zeros(shape[:-2] + (ny - 2 * w, nx - 2 * w),
                        dtype=torch.float64)
        g = torch.zeros_like(o)
        for a in range(2 * w + 1):
            for b in range(2 * w + 1):
                c = k[a, b].item()
                if c == 0.0:
                    continue
                s = v[..., a:ny - 2 * w + a, b:nx - 2 * w + b]
                o = o + c * s
                g = g + abs(c) * s.abs()
        outs.append(o)
        mags.append(g)
    return (outs, mags) if with_mag else outs


def oracle_adjoint_chain(src, weights, gout, dtype, with_mag=False):
    """``A^T`` on one gradient ``gout`` in float64: ``S^T`` by index_add_
    over the taps, rounded to ``dtype`` where the library stores, then
    ``E^T`` over the source map ``src``, rounded again."""
    k = torch.as_tensor(weights, dtype=torch.float64)
    w = (k.shape[0] - 1) // 2
    shape = tuple(gout.shape)
    ny, nx = shape[-2:]
    ids = torch.arange(gout.numel()).reshape(-1, ny, nx)
    g = gout.detach().cpu().double().reshape(-1, ny, nx)
    inner = g[:, w:ny - w, w:nx - w].reshape(-1)
    st = torch.zeros(gout.numel(), dtype=torch.float64)
    mag = torch.zeros_like(st)
    for a in range(2 * w + 1):
        for b in range(2 * w + 1):
            c = k[a, b].item()
            if c == 0.0:
                continue
            dst = ids[:, a:ny - 2 * w + a, b:nx - 2 * w + b].reshape(-1)
            st.index_add_(0, dst, c * inner)
            mag.index_add_(0, dst, abs(c) * inner.abs())
    st = st.to(dtype).double().reshape(shape)
    out = oracle_adjoint(src, st).to(dtype).double()
    if with_mag:
        return out, oracle_adjoint(src, mag.reshape(shape))
    return out


def interior(t, w):
    return t[..., w:t.shape[-2] - w, w:t.shape[-1] - w]


def check_bound(got, exact, mag, n, dtype, what):
    """The a-priori bound of the module docstring, per cell."""
    bound = gamma(n + 2, unit_acc(dtype)) * mag + unit_out(dtype) * \
        exact.abs()
    err = (got.detach().cpu().double() - exact).abs()
    worst = (err - bound).max().item()
    assert worst <= 0.0, (what, "max err", err.max().item(), "over by",
                          worst)


@pytest.fixture(scope="module")
def grids():
    m.init()
    return {p: CartesianGrid(dims=(1, 1), periodic=p) for p in PERIODIC}


# ----------------------------------------------------------------- world 1

SHAPES = [(3, 3), (4, 4), (6, 6), (7, 7), (9, 9), (10, 10), (12, 12),
          (13, 13), (9, 14), (2, 12, 9), (2, 3, 13, 12)]


@pytest.mark.parametrize("periodic", PERIODIC)
@pytest.mark.parametrize("w", [1, 2, 3, 4])
def test_world1_apply_matches_oracle(grids, periodic, w):
    grid = grids[periodic]
    shapes = [s for s in SHAPES if fits(s, w)]
    assert any(s[-1] == 3 * w for s in shapes)
    assert any(s[-1] == 3 * w + 1 for s in shapes)
    ran = 0
    for shape, kind in itertools.product(shapes, KINDS):
        k = make_weights(kind, w)
        for nf, dtype in itertools.product((1, 3), DTYPES):
            st = grid.make_stencil(shape, dtype, "cpu", k, nfields=nf)
            x = [int_data(shape, dtype, 31 * i + nf) for i in range(nf)]
            keep = [f.clone() for f in x]
            exp = oracle_apply(grid, k, x)
            got = as_tuple(st.apply(*x))
            assert len(got) == nf
            for f, kp, o, e in zip(x, keep, got, exp):
                assert torch.equal(f, kp), "apply() mutated its input"
                assert o.dtype == dtype and o.shape == f.shape
                assert torch.equal(interior(o, w).double(),
                                   e.to(dtype).double()), (shape, kind, dtype)
                halo = o.clone()
                interior(halo, w).zero_()
                assert not halo.any(), "out=None must have a zero halo"
            ran += 1
    assert ran == len(shapes) * len(KINDS) * 8


def test_eight_fields_and_one_field_return_types(grids):
    grid = grids[(True, False)]
    shape, w = (2, 9, 10), 2
    k = make_weights("asym", w)
    st = grid.make_stencil(shape, torch.float32, "cpu", k, nfields=8)
    x = [int_data(shape, torch.float32, i) for i in range(8)]
    got = st.apply(*x)
    assert isinstance(got, tuple) and len(got) == 8
    for o, e in zip(got, oracle_apply(grid, k, x)):
        assert torch.equal(interior(o, w).double(), e)
    st1 = grid.make_stencil(shape, torch.float32, "cpu", k)
    assert isinstance(st1.apply(x[0]), torch.Tensor)
    assert isinstance(st1, HaloStencil)
    assert st1.width == 2 and st1.exchanger.width == 2
    assert st1.exchanger.nfields == 1 and st.exchanger.nfields == 8


def test_taps_order_and_zero_drop(grids):
    k = [[0, 1.5, 0], [2, 0, -3], [0, 0, 4]]
    st = grids[(True, True)].make_stencil((5, 5), torch.float32, "cpu", k)
    assert st.taps == [(-1, 0, 1.5), (0, -1, 2.0), (0, 1, -3.0),
                       (1, 1, 4.0)]
    assert st.width == 1
    # a tensor of weights is taken as well
    st2 = grids[(True, True)].make_stencil(
        (5, 5), torch.float32, "cpu", torch.tensor(k, dtype=torch.float32))
    assert st2.taps == st.taps


def test_out_keeps_halos_and_inputs_unmutated(grids):
    for periodic, dtype in itertools.product(PERIODIC, DTYPES):
        grid = grids[periodic]
        shape, w, nf = (2, 9, 10), 2, 2
        k = make_weights("asym", w)
        st = grid.make_stencil(shape, dtype, "cpu", k, nfields=nf)
        x = [int_data(shape, dtype, 3 + i) for i in range(nf)]
        keep = [f.clone() for f in x]
        outs = [torch.full(shape, 7.0, dtype=dtype) for _ in range(nf)]
        ret = st.apply(*x, out=outs)
        ref = as_tuple(st.apply(*x))
        for i in range(nf):
            assert ret[i] is outs[i]
            assert torch.equal(x[i], keep[i])
            assert torch.equal(interior(outs[i], w), interior(ref[i], w))
            halo = outs[i].clone()
            interior(halo, w).fill_(7.0)
            assert torch.equal(halo, torch.full(shape, 7.0, dtype=dtype))
    # one field: a bare tensor as out=
    st1 = grids[(True, True)].make_stencil((9, 10), torch.float32, "cpu",
                                           make_weights("star", 1))
    x = int_data((9, 10), torch.float32, 1)
    o = torch.zeros(9, 10)
    assert st1.apply(x, out=o) is o
    assert torch.equal(o, st1.apply(x))


def test_zero_weight_over_inf_is_finite(grids):
    k = torch.zeros(3, 3, dtype=torch.float64)
    k[1, 2] = 2.0  # reads only the east neighbour
    for periodic in PERIODIC:
        grid = grids[periodic]
        st = grid.make_stencil((5, 6), torch.float32, "cpu", k)
        x = int_data((5, 6), torch.float32, 2)
        x[2, 2] = float("inf")
        out = st.apply(x)
        # (2, 1) reads (2, 2); every other cell must stay finite — also
        # (2, 2) itself, whose own weight is a dropped zero
        assert out[2, 1] == float("inf")
        rest = out.clone()
        rest[2, 1] = 0.0
        assert torch.isfinite(rest).all()
        g = torch.zeros(5, 6)
        g[2, 2] = float("inf")
        gin = st.adjoint(g)
        assert torch.isinf(gin).sum() == 1 and not torch.isnan(gin).any()


@pytest.mark.parametrize("periodic", PERIODIC)
@pytest.mark.parametrize("w", [1, 2, 4])
def test_world1_adjoint_matches_oracle_and_dot_product(grids, periodic, w):
    grid = grids[periodic]
    shapes = [s for s in SHAPES if fits(s, w)]
    for shape, kind in itertools.product(shapes, KINDS):
        k = make_weights(kind, w)
        src = source_map(grid, shape, w)
        for nf, dtype in itertools.product((1, 3), DTYPES):
            st = grid.make_stencil(shape, dtype, "cpu", k, nfields=nf)
            y = [int_data(shape, dtype, 17 * i + nf) for i in range(nf)]
            keep = [g.clone() for g in y]
            gin = as_tuple(st.adjoint(*y))
            for g, kp, o in zip(y, keep, gin):
                assert torch.equal(g, kp), "adjoint() mutated its input"
                assert o.dtype == dtype and o.shape == g.shape
                exp = oracle_adjoint_chain(src, k, g, dtype)
                assert torch.equal(o.double(), exp), (shape, kind, dtype)
            # out= form: every cell is written
            outs = [torch.full(shape, 7.0, dtype=dtype) for _ in range(nf)]
            ret = as_tuple(st.adjoint(*y, out=outs))
            for r, o, gi in zip(ret, outs, gin):
                assert r is o and torch.equal(o, gi)
            if dtype in (torch.float16, torch.bfloat16):
                continue  # a rounded store breaks the exact identity
            # <A x, y> == <x, A^T y>, exact on integer data
            x = [int_data(shape, dtype, 55 + i) for i in range(nf)]
            ax = as_tuple(st.apply(*x))
            lhs = sum((a.double() * b.double()).sum()
                      for a, b in zip(ax, y))
            rhs = sum((a.double() * b.double()).sum()
                      for a, b in zip(x, gin))
            assert lhs == rhs, (shape, kind, dtype)


def test_random_data_within_bound(grids):
    torch.manual_seed(3)
    for periodic, w, dtype in itertools.product(
            PERIODIC, (1, 4),
            (torch.float32, torch.float64, torch.bfloat16)):
        grid = grids[periodic]
        shape = (2, 13, 14)
        k = torch.randn(2 * w + 1, 2 * w + 1, dtype=torch.float64)
        k[0, 0] = 0.0
        n = ntaps(k)
        st = grid.make_stencil(shape, dtype, "cpu", k, nfields=2)
        x = [torch.randn(shape).to(dtype) for _ in range(2)]
        exp, mag = oracle_apply(grid, k, x, with_mag=True)
        for o, e, g in zip(st.apply(*x), exp, mag):
            check_bound(interior(o, w), e, g, n, dtype,
                        ("apply", periodic, w, dtype))


@pytest.mark.parametrize("shape, w", [((3, 3), 1), ((2, 6, 7), 2)])
def test_gradcheck(grids, shape, w):
    torch.manual_seed(6)
    k = torch.randn(2 * w + 1, 2 * w + 1, dtype=torch.float64)
    for periodic in PERIODIC:
        st = grids[periodic].make_stencil(shape, torch.float64, "cpu", k,
                                          nfields=2)
        a = torch.randn(shape, dtype=torch.float64, requires_grad=True)
        b = torch.randn(shape, dtype=torch.float64)
        assert torch.autograd.gradcheck(lambda x: st.apply_ad(x, b), (a,))
        assert torch.autograd.gradcheck(lambda x: st.apply_ad(b, x), (a,))
        out = st.apply_ad(a, b)
        (out[0].sum() + out[1].sum()).backward()
        assert a.grad is not None and b.grad is None
        a.grad = None


def test_apply_ad_values_equal_apply(grids):
    for periodic, dtype in itertools.product(PERIODIC, DTYPES):
        st = grids[periodic].make_stencil(
            (2, 9, 10), dtype, "cpu", make_weights("asym", 2), nfields=2)
        torch.manual_seed(8)
        a = torch.randn(2, 9, 10).to(dtype)
        b = torch.randn(2, 9, 10).to(dtype)
        ref = st.apply(a, b)
        ar = a.clone().requires_grad_()
        out = st.apply_ad(ar, b)
        assert isinstance(out, tuple) and len(out) == 2
        for o, r in zip(out, ref):
            assert torch.equal(o.detach(), r)
        assert torch.equal(ar.detach(), a)
        g = int_data((2, 9, 10), dtype, 5)
        out[0].backward(g)
        assert torch.equal(ar.grad, st.adjoint(g, torch.zeros_like(g))[0])
    st1 = grids[(True, True)].make_stencil((9, 9), torch.float32, "cpu",
                                           make_weights("star", 1))
    x = torch.randn(9, 9, requires_grad=True)
    y = st1.apply_ad(x)
    assert isinstance(y, torch.Tensor)
    y.sum().backward()  # an expanded, non-contiguous incoming gradient
    assert torch.equal(x.grad, st1.adjoint(torch.ones(9, 9)))
    # once differentiable
    x = torch.randn(9, 9, requires_grad=True)
    (gx,) = torch.autograd.grad((st1.apply_ad(x) ** 2).sum(), x,
                                create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable|twice"):
        gx.sum().backward()


def reference_chain(ex, weights, x, steps):
    """``steps`` rounds of exchange_ad + the tap sum by slicing, padded
    back with a zero halo: what ``apply_ad`` computes, under autograd."""
    k = torch.as_tensor(weights, dtype=torch.float64)
    w = (k.shape[0] - 1) // 2
    ny, nx = x.shape[-2:]
    u = x
    for _ in range(steps):
        e = ex.exchange_ad(u)
        acc = None
        for a in range(2 * w + 1):
            for b in range(2 * w + 1):
                c = k[a, b].item()
                if c == 0.0:
                    continue
                term = c * e[..., a:ny - 2 * w + a, b:nx - 2 * w + b]
                acc = term if acc is None else acc + term
        u = F.pad(acc, (w, w, w, w))
    return u


def chain_gradients(grid, weights, x, g, steps=3, device="cpu"):
    """(gradient through apply_ad, gradient through the reference) of
    ``sum(u_steps * g)`` with respect to ``x``."""
    k = torch.as_tensor(weights, dtype=torch.float64)
    w = (k.shape[0] - 1) // 2
    st = grid.make_stencil(x.shape, x.dtype, device, k)
    x1 = x.clone().to(device).requires_grad_()
    u = x1
    for _ in range(steps):
        u = st.apply_ad(u)
    (u * g.to(device)).sum().backward()
    ex = grid.make_halo_exchanger(x.shape, x.dtype, "cpu", width=w)
    x2 = x.clone().requires_grad_()
    (reference_chain(ex, k, x2, steps) * g).sum().backward()
    return x1.grad.cpu(), x2.grad


def test_gradient_through_three_steps_equals_autograd(grids):
    """Integer data: bitwise (the largest partial sum is below
    (sum|K|)^3 * 9^3 * 4 < 2^53).  Random data: both gradients carry at
    most 3 * (n + 2 + 9) roundings per term (per step n taps, one product,
    one coefficient, and up to 9 adds in the exchange's adjoint), so they
    differ by at most 2 * gamma(3 * (n + 11)) * (|A|^T)^3 |g|, the last
    factor from the reference chain run on absolute values."""
    shape, w = (2, 9, 10), 2
    for periodic, kind in itertools.product(PERIODIC, ("star", "asym")):
        grid = grids[periodic]
        k = make_weights(kind, w)
        x = int_data(shape, torch.float64, 1)
        g = int_data(shape, torch.float64, 2)
        got, ref = chain_gradients(grid, k, x, g)
        assert torch.equal(got, ref), (periodic, kind)
        assert got.abs().max() > 0
    torch.manual_seed(4)
    for periodic in PERIODIC:
        grid = grids[periodic]
        k = torch.randn(5, 5, dtype=torch.float64)
        x = torch.randn(shape, dtype=torch.float64)
        g = torch.randn(shape, dtype=torch.float64)
        got, ref = chain_gradients(grid, k, x, g)
        _, mag = chain_gradients(grid, k.abs(), x, g.abs())
        bound = 2 * gamma(3 * (ntaps(k) + 11), 2.0 ** -53) * mag
        assert ((got - ref).abs() <= bound).all(), periodic


def test_errors(grids):
    grid = grids[(True, True)]
    ok = make_weights("star", 1)
    for bad in ([1.0, 2.0, 3.0], torch.zeros(3, 5), torch.zeros(2, 2),
                torch.zeros(4, 4), torch.zeros(3, 3, 3)):
        with pytest.raises(ValueError, match="2r\\+1"):
            grid.make_stencil((9, 9), torch.float32, "cpu", bad)
    for n in (1, 11):
        with pytest.raises(ValueError, match="radius"):
            grid.make_stencil((40, 40), torch.float32, "cpu",
                              torch.ones(n, n))
    with pytest.raises(ValueError, match="non-zero"):
        grid.make_stencil((9, 9), torch.float32, "cpu", torch.zeros(3, 3))
    for dtype in (torch.int32, torch.int64, torch.complex64, torch.uint8):
        with pytest.raises(TypeError, match="float16, bfloat16"):
            grid.make_stencil((9, 9), dtype, "cpu", ok)
    with pytest.raises(ValueError, match="3\\*width"):
        grid.make_stencil((9, 5), torch.float32, "cpu", torch.ones(5, 5))

    st = grid.make_stencil((2, 9, 9), torch.float32, "cpu", ok, nfields=2)
    a = torch.zeros(2, 9, 9)
    b = torch.zeros(2, 9, 9)
    g = torch.zeros(2, 9, 9, requires_grad=True)
    for fn in (st.apply, st.adjoint):
        with pytest.raises(ValueError, match="not differentiable"):
            fn(a, g)
    for fn in (st.apply, st.adjoint, st.apply_ad):
        with pytest.raises(ValueError, match="2 field"):
            fn(a)
        with pytest.raises(ValueError, match="2 field"):
            fn(a, b, a)
        with pytest.raises(ValueError, match="shape"):
            fn(a, torch.zeros(2, 9, 10))
        with pytest.raises(TypeError, match="dtype"):
            fn(a, b.double())
        with pytest.raises(ValueError, match="contiguous"):
            fn(a, torch.zeros(2, 9, 18)[..., ::2])
    big = torch.zeros(3, 2, 9, 9)
    for fn in (st.apply, st.adjoint):
        with pytest.raises(ValueError, match="overlaps input"):
            fn(a, b, out=(a, torch.zeros(2, 9, 9)))
        with pytest.raises(ValueError, match="overlaps input"):
            fn(big[0], big[1], out=(big[2], big[1]))
        with pytest.raises(ValueError, match="overlaps out"):
            fn(a, b, out=(big[0], big[0]))
        with pytest.raises(ValueError, match="2 field"):
            fn(a, b, out=big[0])
        with pytest.raises(ValueError, match="shape"):
            fn(a, b, out=(big[0], torch.zeros(2, 9, 10)))
        with pytest.raises(TypeError, match="dtype"):
            fn(a, b, out=(big[0], big[1].double()))
        with pytest.raises(ValueError, match="contiguous"):
            fn(a, b, out=(big[0], torch.zeros(2, 9, 18)[..., ::2]))
        fn(big[0], big[1], out=(big[2], a))  # neighbours, not overlapping
    assert not a.any() and not big.any()


# --------------------------------------------------------- worlds 2 and 4

BY, BX = 6, 8  # block of interior cells per rank


def _block(grid, dims, t):
    cy, cx = grid.coords
    return t[..., cy * BY:(cy + 1) * BY, cx * BX:(cx + 1) * BX]


def _multirank(rank, ws):
    comm = m.get_world()
    dtype = torch.float64
    for dims, periodic, w in itertools.product(DIMS[ws], PERIODIC, (1, 2)):
        grid = CartesianGrid(comm=comm, dims=dims, periodic=periodic)
        one = fake_grid(0, (1, 1), periodic)
        gy, gx = BY * dims[0], BX * dims[1]
        k = make_weights("asym", w, seed=1)
        # the same global integer fields on every rank, zero halos
        G = [F.pad(int_data((3, gy, gx), dtype, 40 + i), (w, w, w, w))
             for i in range(2)]
        Y = [int_data((3, gy, gx), dtype, 50 + i) for i in range(2)]
        x = [F.pad(_block(grid, dims, interior(g, w)), (w, w, w, w))
             .contiguous() for g in G]
        st = grid.make_stencil(x[0].shape, dtype, "cpu", k, nfields=2)
        st1 = one.make_stencil(G[0].shape, dtype, "cpu", k, nfields=2)

        # decomposed apply == single-domain apply on the global field
        got = st.apply(*x)
        ref = st1.apply(*G)
        for o, r in zip(got, ref):
            assert torch.equal(interior(o, w),
                               _block(grid, dims, interior(r, w))), \
                (dims, periodic, w, rank)

        # allreduced <A x, y> == <x, A^T y>
        y = [F.pad(_block(grid, dims, t), (w, w, w, w)).contiguous()
             for t in Y]
        gin = st.adjoint(*y)
        lhs = sum((a * b).sum() for a, b in zip(got, y))
        rhs = sum((a * b).sum() for a, b in zip(x, gin))
        lhs = m.allreduce(lhs, m.SUM, comm=comm)
        rhs = m.allreduce(rhs, m.SUM, comm=comm)
        assert lhs == rhs and lhs != 0, (dims, periodic, w, rank)

        # gradient of sum(u_3 * T) through 3 steps == the single-domain one
        def grad(stn, interior0, target):
            x0 = interior0.clone().requires_grad_()
            z = torch.zeros_like(x0)
            u, v = F.pad(x0, (w, w, w, w)), F.pad(z, (w, w, w, w))
            for _ in range(3):
                u, v = stn.apply_ad(u, v)
            (interior(u, w) * target).sum().backward()
            return x0.grad

        gl = grad(st, _block(grid, dims, interior(G[0], w)),
                  _block(grid, dims, Y[0]))
        gg = grad(st1, interior(G[0], w), Y[0])
        assert torch.equal(gl, _block(grid, dims, gg)), \
            (dims, periodic, w, rank)
        assert gg.abs().max() > 0


@pytest.mark.parametrize("ws", [2, 4])
def test_multirank_apply_dot_product_and_gradient(ws):
    """One spawn per world size."""
    run_multiproc(_multirank, ws)


# ----------------------------------------------------------------- example

@pytest.mark.parametrize("n", [1, 2])
def test_fused_stencil_example(n):
    cmd = [sys.executable, "examples/fused_stencil_diffusion.py",
           "--size", "24", "--nz", "2", "--steps", "6", "--grad-steps", "4",
           "--descent", "3", "--device", "cpu"]
    if n > 1:
        cmd = [sys.executable, "-m", "mpi4jax_amd.run", "-n", str(n)] + cmd[1:]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300,
                         env=ENV, cwd=REPO)
    assert res.returncode == 0, res.stderr + res.stdout
    assert f"OK: 6 fused steps and a gradient through 4 over {n} rank(s)" \
        in res.stdout
    before = float(re.search(r"loss before: (\S+)", res.stdout).group(1))
    after = float(re.search(r"loss after 3 descent steps: (\S+)",
                            res.stdout).group(1))
    assert after < before
