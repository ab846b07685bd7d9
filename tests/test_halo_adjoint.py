"""CPU suite for the adjoint of parallel/halo.HaloExchanger:
``adjoint`` / ``adjoint_`` and the differentiable ``exchange_ad``.

The oracle is built from the forward exchanger itself.  An exchange only
copies, so running it on an int64 field of global cell ids gives, for
every output cell, the id of the input cell it read.  The forward pass is
then ``out = in[src]`` and its adjoint is
``gin = zeros.index_add_(0, src, gout)``.

Comparisons against the oracle use integer-valued data from [-4, 4]: a
cell collects at most 9 terms, so every sum is exact in all four dtypes
and the comparison is bitwise whatever the order of the adds.
"""

import itertools
import re
import subprocess
import sys

import pytest
import torch

import mpi4jax_amd as m
from mpi4jax_amd.parallel.grid import CartesianGrid
from _mp import run_multiproc
from test_halo_exchanger import (DIMS, ENV, PERIODIC, REPO, TOPOLOGIES,
                                 fake_grid)

WRAPPING = [(True, True), (False, True), (True, False)]
SHAPES = [(3, 3), (6, 6), (9, 9), (9, 10), (12, 9), (6, 131), (2, 9, 13),
          (2, 3, 9, 10)]
DTYPES = (torch.float64, torch.float32, torch.bfloat16, torch.float16)


def _fits(shape, w):
    return shape[-2] >= 3 * w and shape[-1] >= 3 * w


def _as_tuple(out):
    return out if isinstance(out, tuple) else (out,)


def int_data(shape, dtype, seed, device="cpu"):
    """Integer values in [-4, 4], exactly representable in ``dtype``."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-4, 5, shape, generator=g).to(dtype).to(device)


def source_map(grid, shape, w):
    """Flat index of the pre-exchange cell every output cell reads
    (world 1)."""
    n = 1
    for s in shape:
        n *= s
    ids = torch.arange(n, dtype=torch.int64).reshape(shape)
    ex = grid.make_halo_exchanger(shape, torch.int64, "cpu", width=w)
    return ex.exchange(ids).reshape(-1)


def oracle_adjoint(src, gout):
    """``gin`` of ``out = in[src]`` for one field, summed in float64."""
    flat = gout.detach().cpu().double().reshape(-1)
    return torch.zeros_like(flat).index_add_(0, src, flat).reshape(
        gout.shape)


@pytest.fixture(scope="module")
def grids():
    m.init()
    return {p: CartesianGrid(dims=(1, 1), periodic=p) for p in PERIODIC}


# ----------------------------------------------------------------- world 1

@pytest.mark.parametrize("periodic", PERIODIC)
@pytest.mark.parametrize("w", [1, 2, 3])
def test_world1_adjoint_matches_oracle_and_dot_product(grids, periodic, w):
    grid = grids[periodic]
    shapes = [s for s in SHAPES if _fits(s, w)]
    # the shapes where the west and east send windows coincide
    assert any(s[-1] == 3 * w and s[-2] == 3 * w for s in shapes)
    ran = 0
    for shape in shapes:
        src = source_map(grid, shape, w)
        for nf, dtype in itertools.product((1, 3), DTYPES):
            ex = grid.make_halo_exchanger(shape, dtype, "cpu", width=w,
                                          nfields=nf)
            gout = [int_data(shape, dtype, 10 * k + nf) for k in range(nf)]
            keep = [g.clone() for g in gout]
            gin = _as_tuple(ex.adjoint(*gout))
            for g, k, o in zip(gout, keep, gin):
                assert torch.equal(g, k), "adjoint() mutated its input"
                assert o.dtype == dtype and o.shape == g.shape
                assert torch.equal(o.double(), oracle_adjoint(src, g)), \
                    (shape, nf, dtype)
            # in-place form: same result, returns the tensors themselves
            ret = _as_tuple(ex.adjoint_(*gout))
            for g, r, o in zip(gout, ret, gin):
                assert r is g and torch.equal(g, o)
            # <exchange(x), y> == <x, adjoint(y)>, exact on integer data
            x = [int_data(shape, dtype, 77 + k) for k in range(nf)]
            fx = _as_tuple(ex.exchange(*x))
            lhs = sum((a.double() * b.double()).sum() for a, b in
                      zip(fx, keep))
            rhs = sum((a.double() * b.double()).sum() for a, b in
                      zip(x, gin))
            assert lhs == rhs, (shape, nf, dtype)
            ran += 1
    assert ran == len(shapes) * 8


def test_closed_grid_adjoint_is_the_identity(grids):
    ex = grids[(False, False)].make_halo_exchanger(
        (2, 9, 10), torch.float32, "cpu", width=2, nfields=2)
    g = [torch.randn(2, 9, 10) for _ in range(2)]
    for a, b in zip(ex.adjoint(*g), g):
        assert torch.equal(a, b)


@pytest.mark.parametrize("periodic", WRAPPING)
def test_width1_equals_autograd_through_halo_exchange(grids, periodic):
    """Bitwise on random data, which pins the order of the adds: the
    interior corner cells collect four terms (all nine at (3, 3)), and
    with the entries taken forwards instead of backwards they come out an
    ulp off for some seeds (seed 4 at (9, 11) is one).  50 seeds per
    shape, so the match does not hang on one draw."""
    grid = grids[periodic]
    for shape, seed in itertools.product([(9, 11), (3, 3)], range(50)):
        torch.manual_seed(seed)
        a = torch.randn(shape, dtype=torch.float64)
        g = torch.randn(shape, dtype=torch.float64)
        ex = grid.make_halo_exchanger(a.shape, a.dtype, "cpu")
        a1 = a.clone().requires_grad_()
        ex.exchange_ad(a1).backward(g)
        a2 = a.clone().requires_grad_()
        grid.halo_exchange(a2).backward(g)
        assert torch.equal(a1.grad, a2.grad), (shape, seed)
        assert torch.equal(a1.grad, ex.adjoint(g)), (shape, seed)


@pytest.mark.parametrize("shape, w", [((3, 3), 1), ((2, 6, 7), 2)])
def test_gradcheck(grids, shape, w):
    """(3, 3) admits width 1 only (n >= 3*width); (2, 6, 7) runs at
    width 2 with ny == 3*width."""
    torch.manual_seed(6)
    for periodic in PERIODIC:
        ex = grids[periodic].make_halo_exchanger(
            shape, torch.float64, "cpu", width=w, nfields=2)
        a = torch.randn(shape, dtype=torch.float64, requires_grad=True)
        b = torch.randn(shape, dtype=torch.float64)
        # only one of the two fields requires grad
        assert torch.autograd.gradcheck(lambda x: ex.exchange_ad(x, b),
                                        (a,))
        assert torch.autograd.gradcheck(lambda x: ex.exchange_ad(b, x),
                                        (a,))
        out = ex.exchange_ad(a, b)
        (out[0].sum() + out[1].sum()).backward()
        assert a.grad is not None and b.grad is None
        a.grad = None


def test_gradcheck_width2_on_6x6(grids):
    """Width 2 at n == 3*width: the west and east windows coincide."""
    torch.manual_seed(7)
    ex = grids[(True, True)].make_halo_exchanger(
        (6, 6), torch.float64, "cpu", width=2, nfields=2)
    a = torch.randn(6, 6, dtype=torch.float64, requires_grad=True)
    b = torch.randn(6, 6, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(ex.exchange_ad, (a, b))


def test_exchange_ad_forward_values_and_unused_output(grids):
    for periodic, dtype in itertools.product(PERIODIC, DTYPES):
        ex = grids[periodic].make_halo_exchanger(
            (2, 9, 10), dtype, "cpu", width=2, nfields=2)
        torch.manual_seed(8)
        a = torch.randn(2, 9, 10).to(dtype)
        b = torch.randn(2, 9, 10).to(dtype)
        ref = ex.exchange(a, b)
        ar = a.clone().requires_grad_()
        out = ex.exchange_ad(ar, b)
        assert isinstance(out, tuple) and len(out) == 2
        for o, r in zip(out, ref):
            assert torch.equal(o.detach(), r)
        assert torch.equal(ar.detach(), a), "exchange_ad mutated its input"
        # the loss looks at one output only: the other's gradient arrives
        # as zeros
        g = int_data((2, 9, 10), dtype, 5)
        out[0].backward(g)
        exp = ex.adjoint(g, torch.zeros_like(g))[0]
        assert torch.equal(ar.grad, exp)
    # one field in, one tensor out
    ex1 = grids[(True, True)].make_halo_exchanger((9, 9), torch.float32,
                                                  "cpu")
    x = torch.randn(9, 9, requires_grad=True)
    y = ex1.exchange_ad(x)
    assert isinstance(y, torch.Tensor)
    assert torch.equal(y.detach(), ex1.exchange(x.detach()))
    # a non-contiguous (expanded) incoming gradient
    y.sum().backward()
    assert torch.equal(x.grad, ex1.adjoint(torch.ones(9, 9)))


def test_errors(grids):
    grid = grids[(True, True)]
    ex = grid.make_halo_exchanger((2, 9, 9), torch.float32, "cpu", width=2,
                                  nfields=2)
    a = torch.zeros(2, 9, 9)
    g = torch.zeros(2, 9, 9, requires_grad=True)
    # the non-differentiable entries still say so
    with pytest.raises(ValueError,
                       match="not differentiable.*halo_exchange"):
        ex.exchange(a, g)
    with pytest.raises(ValueError, match="not differentiable"):
        ex.exchange_(a, g)
    for fn in (ex.exchange_ad, ex.adjoint, ex.adjoint_):
        with pytest.raises(ValueError, match="2 field"):
            fn(a)
        with pytest.raises(ValueError, match="2 field"):
            fn(a, a, a)
        with pytest.raises(ValueError, match="shape"):
            fn(a, torch.zeros(2, 9, 10))
        with pytest.raises(ValueError, match="contiguous"):
            fn(a, torch.zeros(2, 9, 18)[..., ::2])
        with pytest.raises(TypeError, match="dtype"):
            fn(a, a.double())
        with pytest.raises(TypeError, match="Tensor"):
            fn(a, 1.0)
    for dtype in (torch.int32, torch.int64, torch.complex64, torch.uint8):
        exi = grid.make_halo_exchanger((9, 9), dtype, "cpu")
        z = torch.zeros(9, 9, dtype=dtype)
        for fn in (exi.exchange_ad, exi.adjoint, exi.adjoint_):
            with pytest.raises(
                    TypeError,
                    match="float16, bfloat16, float32 and float64"):
                fn(z)
        assert torch.equal(exi.exchange(z), z)  # forward-only still works
    assert torch.equal(a, torch.zeros(2, 9, 9))

    # double backward raises
    ex1 = grid.make_halo_exchanger((9, 9), torch.float64, "cpu")
    x = torch.randn(9, 9, dtype=torch.float64, requires_grad=True)
    y = ex1.exchange_ad(x)
    (gx,) = torch.autograd.grad((y * y).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable|twice"):
        gx.sum().backward()


# --------------------------------------------------------- worlds 2 and 4

def _stencil_step(u, w=2):
    """Width-2 update touching the axis neighbours at distance 1 and 2 and
    the four distance-2 diagonals (a copy of the one in
    tests/test_halo_exchanger.py)."""
    c = u[..., 2:-2, 2:-2]
    lap = ((-u[..., 2:-2, :-4] + 16.0 * u[..., 2:-2, 1:-3] - 30.0 * c
            + 16.0 * u[..., 2:-2, 3:-1] - u[..., 2:-2, 4:]) / 12.0
           + (-u[..., :-4, 2:-2] + 16.0 * u[..., 1:-3, 2:-2] - 30.0 * c
              + 16.0 * u[..., 3:-1, 2:-2] - u[..., 4:, 2:-2]) / 12.0)
    diag = (u[..., :-4, :-4] + u[..., :-4, 4:] + u[..., 4:, :-4]
            + u[..., 4:, 4:] - 4.0 * c)
    new = u.clone()
    new[..., 2:-2, 2:-2] = c + 0.05 * lap + 0.01 * diag
    return new


def _multirank_oracle(rank, ws):
    comm = m.get_world()
    by, bx, nf, dtype = 6, 8, 2, torch.float64
    for dims, periodic, w in itertools.product(DIMS[ws], PERIODIC, (1, 2)):
        grid = CartesianGrid(comm=comm, dims=dims, periodic=periodic)
        shape = (3, by + 2 * w, bx + 2 * w)
        n = shape[0] * shape[1] * shape[2]
        ids = (rank * n + torch.arange(n, dtype=torch.int64)).reshape(shape)
        exi = grid.make_halo_exchanger(shape, torch.int64, "cpu", width=w)
        src = exi.exchange(ids).reshape(-1)
        ex = grid.make_halo_exchanger(shape, dtype, "cpu", width=w,
                                      nfields=nf)
        gout = [int_data(shape, dtype, 1000 * rank + k) for k in range(nf)]
        keep = [g.clone() for g in gout]
        gin = ex.adjoint(*gout)

        src_all = m.allgather(src, comm=comm).reshape(-1)
        for k in range(nf):
            assert torch.equal(gout[k], keep[k])
            g_all = m.allgather(gout[k], comm=comm).reshape(-1)
            exp = torch.zeros(ws * n, dtype=dtype).index_add_(
                0, src_all, g_all)[rank * n:(rank + 1) * n].reshape(shape)
            assert torch.equal(gin[k], exp), (dims, periodic, w, rank, k)

        # <exchange(x), y> == <x, adjoint(y)> summed over all ranks
        x = [int_data(shape, dtype, 5000 + 10 * rank + k) for k in range(nf)]
        fx = ex.exchange(*x)
        lhs = sum((a * b).sum() for a, b in zip(fx, gout))
        rhs = sum((a * b).sum() for a, b in zip(x, gin))
        lhs = m.allreduce(lhs, m.SUM, comm=comm)
        rhs = m.allreduce(rhs, m.SUM, comm=comm)
        assert lhs == rhs, (dims, periodic, w, rank)


def _loss_gradient(grid, dims, G, T, k=3):
    """Gradient of sum((u_k - T)^2) with respect to this rank's block of
    G, through k rounds of exchange_ad + the width-2 stencil."""
    w = 2
    by, bx = G.shape[-2] // dims[0], G.shape[-1] // dims[1]
    cy, cx = grid.coords
    blk = (slice(None), slice(cy * by, (cy + 1) * by),
           slice(cx * bx, (cx + 1) * bx))
    u0 = G[blk].clone().requires_grad_()
    u = torch.nn.functional.pad(u0, (w, w, w, w))
    ex = grid.make_halo_exchanger(u.shape, u.dtype, "cpu", width=w)
    for _ in range(k):
        u = _stencil_step(ex.exchange_ad(u))
    loss = ((u[:, w:-w, w:-w] - T[blk]) ** 2).sum()
    loss.backward()  # the local term; the adjoints carry the rest across
    return u0.grad


def _multirank_loss(rank, ws):
    """Not bitwise: a cell next to a block edge sums the same terms in
    another association (in world 1 they all come from the stencil's
    backward pass; in a decomposed run some arrive through the adjoint's
    adds).  Every entry must equal the world-1 entry to rtol 1e-12, plus
    an absolute floor of 8 ulp of the gradient's largest entry
    (8 * eps * max|ref|, about 7e-15 here).  The floor is there because an
    entry is a sum of terms of the size of the largest entries and may
    cancel to almost nothing, while a reassociated add is off by up to
    one ulp of its operands, not of the result; a cell collects at most 9
    terms, so at most 8 adds change place.  Measured at 2 and 4 ranks:
    max |diff| 1.3e-15 against entries up to 3.9; without the floor one entry
    of 2.4e-5, off by 3e-17, has a ratio of 1.2e-12."""
    comm = m.get_world()
    torch.manual_seed(12)  # same global fields on every rank
    G = torch.randn(2, 24, 24, dtype=torch.float64)
    T = torch.randn(2, 24, 24, dtype=torch.float64)
    for periodic in PERIODIC:
        ref = _loss_gradient(fake_grid(0, (1, 1), periodic), (1, 1), G, T)
        for dims in DIMS[ws]:
            grid = CartesianGrid(comm=comm, dims=dims, periodic=periodic)
            got = _loss_gradient(grid, dims, G, T)
            by, bx = 24 // dims[0], 24 // dims[1]
            cy, cx = grid.coords
            mine = ref[:, cy * by:(cy + 1) * by, cx * bx:(cx + 1) * bx]
            err = (got - mine).abs().max().item()
            scale = ref.abs().max().item()
            floor = 8 * torch.finfo(torch.float64).eps * scale
            print(f"loss gradient {dims} {periodic} r{rank}: "
                  f"max |diff| {err:.3e}, max |ref| {scale:.3e}, "
                  f"floor {floor:.3e}")
            torch.testing.assert_close(
                got, mine, rtol=1e-12, atol=floor,
                msg=lambda s: f"{dims} {periodic} r{rank}: {s}")


def _multirank_all(rank, ws):
    _multirank_oracle(rank, ws)
    _multirank_loss(rank, ws)


@pytest.mark.parametrize("ws", [2, 4])
def test_multirank_oracle_dot_product_and_loss_gradient(ws):
    """One spawn per world size: the global index-map oracle, the
    allreduced dot-product identity, and the gradient of a loss through
    three rounds of exchange_ad + a width-2 stencil against the same
    block of the world-1 gradient."""
    run_multiproc(_multirank_all, ws)


# -------------------------------------------- schedule matching, no procs

@pytest.mark.parametrize("dims", TOPOLOGIES)
def test_adjoint_schedule_cross_rank_matching(dims):
    size = dims[0] * dims[1]
    for periodic, w, nf, force in itertools.product(
            PERIODIC, (1, 3), (1, 3), (False, True)):
        sends, recvs = {}, {}
        for rank in range(size):
            ex = fake_grid(rank, dims, periodic).make_halo_exchanger(
                (2, 9, 10), torch.float32, "cpu", width=w, nfields=nf,
                _force_remote=force)
            local = set(ex.local_directions)
            fwd, adj = ex.schedule(), ex.adjoint_schedule()
            assert len(fwd) == len(adj)
            for (d, st, rf, n), (d2, st2, rf2, n2) in zip(fwd, adj):
                # same entries, same order, roles swapped
                assert (d2, st2, rf2, n2) == (d, rf, st, n)
                if d in local:
                    continue
                if st2 is not None:
                    sends.setdefault((rank, st2), []).append(n2)
                if rf2 is not None:
                    recvs.setdefault((rank, rf2), []).append(n2)
        pairs = set(sends) | {(s, d) for (d, s) in recvs}
        for src, dst in pairs:
            assert sends.get((src, dst), []) == recvs.get((dst, src), []), \
                (dims, periodic, w, nf, src, dst)


# ----------------------------------------------------------------- example

@pytest.mark.parametrize("n", [1, 2])
def test_halo_adjoint_example(n):
    cmd = [sys.executable, "examples/halo_adjoint_diffusion.py",
           "--size", "24", "--nz", "2", "--steps", "4", "--descent", "3",
           "--device", "cpu"]
    if n > 1:
        cmd = [sys.executable, "-m", "mpi4jax_amd.run", "-n", str(n)] + cmd[1:]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300,
                         env=ENV, cwd=REPO)
    assert res.returncode == 0, res.stderr + res.stdout
    assert f"OK: gradient through 4 halo exchanges over {n} rank(s)" \
        in res.stdout
    before = float(re.search(r"loss before: (\S+)", res.stdout).group(1))
    after = float(re.search(r"loss after 3 descent steps: (\S+)",
                            res.stdout).group(1))
    assert after < before
