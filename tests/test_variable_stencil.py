"""CPU suite for parallel/varstencil.VariableHaloStencil
(``CartesianGrid.make_variable_stencil``), and the helpers it shares with
tests/test_gpu_variable_stencil.py.

Oracle: ``HaloExchanger.exchange`` of the fields in float64 on the CPU,
then ``sum_t K_t * shifted slice`` in float64 (``oracle``).  Integer fields
in [-4, 4] with integer coefficients in [-3, 3] keep every partial sum of
at most 13 taps within 156, exact in every dtype, so those results are
compared bitwise.  The halo of every coefficient tensor is NaN: no result
may depend on it.
"""

import itertools

import pytest
import torch
import torch.nn.functional as F

import mpi4jax_amd as m
from mpi4jax_amd.parallel import VariableHaloStencil
from mpi4jax_amd.parallel.grid import CartesianGrid
from test_halo_adjoint import int_data
from test_halo_exchanger import PERIODIC
from test_halo_stencil import as_tuple, check_bound, interior
from test_stencil_cg import int_dot

DTYPES = (torch.float64, torch.float32, torch.bfloat16, torch.float16)
TAPSETS = {
    "single": [(1, -1)],
    "star5": [(0, 0), (-1, 0), (0, -1), (0, 1), (1, 0)],
    "box9": list(itertools.product((-1, 0, 1), repeat=2)),
    "star13": [(0, 0)] + [o for d in (1, 2, 3)
                          for o in ((-d, 0), (d, 0), (0, -d), (0, d))],
    "asym4": [(4, -1), (0, 0), (-2, 3), (-4, 4), (1, 2), (0, -4)],
}
SOLVES = [(torch.float64, 1e-10, 80), (torch.float32, 1e-5, 40)]


def radius(offsets):
    return max(max(abs(dy), abs(dx)) for dy, dx in offsets)


def shapes_for(w):
    """The smallest plane, a ragged multi-tile one, and one with a
    fast-fill tile at every width over five levels."""
    return [(3 * w, 3 * w + 1), (3, 41, 70), (5, 76, 140)]


def nan_halo(k, w):
    out = torch.full_like(k, float("nan"))
    interior(out, w).copy_(interior(k, w))
    return out


def int_coef(offsets, shape, seed):
    """Integer coefficients in [-3, 3], different per tap and per cell."""
    g = torch.Generator().manual_seed(1000 + seed)
    k = torch.randint(-3, 4, (len(offsets),) + tuple(shape[-2:]),
                      generator=g).double()
    return nan_halo(k, radius(offsets))


def oracle(grid, offsets, coef, fields, with_mag=False):
    """Interior of ``A`` on ``fields`` in float64 (and
    ``sum_t |K_t| |x_t|``)."""
    w = radius(offsets)
    shape = tuple(fields[0].shape)
    ny, nx = shape[-2:]
    ex = grid.make_halo_exchanger(shape, torch.float64, "cpu", width=w,
                                  nfields=len(fields))
    ki = interior(coef.detach().cpu().double(), w)
    outs, mags = [], []
    for v in as_tuple(ex.exchange(*(f.detach().cpu().double()
                                    for f in fields))):
        s = [v[..., w + dy:ny - w + dy, w + dx:nx - w + dx]
             for dy, dx in offsets]
        outs.append(sum(k * x for k, x in zip(ki, s)))
        mags.append(sum(k.abs() * x.abs() for k, x in zip(ki, s)))
    return (outs, mags) if with_mag else outs


def diffusion_system(grid, dtype, device="cpu"):
    """``I - div(k grad)`` on a 12 x 14 interior, 2 levels: the stencil,
    its float64 coefficients and a right-hand side with a zero halo."""
    offsets = TAPSETS["star5"]
    g = torch.Generator().manual_seed(5)
    k = 0.5 + 1.5 * torch.rand(14, 16, generator=g, dtype=torch.float64)
    k = grid.make_halo_exchanger(k.shape, k.dtype, "cpu").exchange(k)
    coef = torch.zeros(5, 14, 16, dtype=torch.float64)
    for t, (dy, dx) in enumerate(offsets[1:], 1):
        interior(coef[t], 1).copy_(
            -(interior(k, 1) + k[1 + dy:13 + dy, 1 + dx:15 + dx]) / 2)
    coef[0] = 1 - coef[1:].sum(0)
    coef = nan_halo(coef, 1)
    b = F.pad(torch.randn(2, 12, 14, generator=g, dtype=torch.float64),
              (1, 1, 1, 1)).to(dtype).to(device)
    st = grid.make_variable_stencil(b.shape, dtype, device, offsets, coef)
    return st, coef, b


def check_cg(grid, dtype, rtol, cap, device="cpu"):
    """The acceptance of tests/test_stencil_cg.py::test_solve_table, with
    the true residual recomputed by the float64 oracle."""
    st, coef, b = diffusion_system(grid, dtype, device)
    x, info = st.make_cg().solve(b, rtol=rtol, maxiter=cap, check_every=1)
    assert info.converged is True and info.iterations <= cap
    assert info.residual_norm <= rtol * info.rhs_norm
    (ax,) = oracle(grid, st.offsets, coef, [x])
    bi = interior(b.cpu().double(), 1)
    true = ((bi - ax).norm() / bi.norm()).item()
    print(dtype, device, info.iterations, true / rtol)
    assert true <= 2 * rtol, (dtype, true)
    return st, b, x


@pytest.fixture(scope="module")
def grids():
    m.init()
    return {p: CartesianGrid(dims=(1, 1), periodic=p) for p in PERIODIC}


@pytest.mark.parametrize("periodic", PERIODIC)
@pytest.mark.parametrize("name", list(TAPSETS))
def test_apply_exact_and_adjoint_identity(grids, periodic, name):
    grid, offsets = grids[periodic], TAPSETS[name]
    w = radius(offsets)
    for shape, nf in itertools.product(shapes_for(w), (1, 3)):
        coef = int_coef(offsets, shape, nf)
        base = [int_data(shape, torch.float64, 7 * i + nf) for i in range(nf)]
        exp = oracle(grid, offsets, coef, base)
        for dtype in DTYPES:
            st = grid.make_variable_stencil(shape, dtype, "cpu", offsets,
                                            coef, nfields=nf)
            assert isinstance(st, VariableHaloStencil) and st.width == w
            x = [f.to(dtype) for f in base]
            got = as_tuple(st.apply(*x))
            for o, e, f, k in zip(got, exp, x, base):
                assert torch.equal(f.double(), k), "apply() mutated its input"
                assert torch.equal(interior(o, w).double(), e), (shape, dtype)
            y = [int_data(shape, dtype, 50 + i) for i in range(nf)]
            gin = as_tuple(st.adjoint(*y))
            assert all(torch.isfinite(g).all() for g in gin)
            if dtype in (torch.float32, torch.float64):
                assert (sum(int_dot(a, b) for a, b in zip(got, y))
                        == sum(int_dot(a, b) for a, b in zip(x, gin)))
                out, pap = st.apply_dot(*x)
                assert all(torch.equal(a, b)
                           for a, b in zip(as_tuple(out), got))
                assert pap.item() == sum(int_dot(a, b)
                                         for a, b in zip(x, got))


@pytest.mark.parametrize("dtype", DTYPES)
def test_rounding_within_bound(grids, dtype):
    torch.manual_seed(17)
    offsets, shape = TAPSETS["box9"], (2, 76, 140)
    coef = nan_halo(torch.randn(9, 76, 140, dtype=torch.float64), 1)
    for periodic in PERIODIC:
        x = [torch.randn(shape).to(dtype)]
        st = grids[periodic].make_variable_stencil(shape, dtype, "cpu",
                                                   offsets, coef)
        (e,), (g,) = oracle(grids[periodic], offsets, coef, x, with_mag=True)
        check_bound(interior(st.apply(*x), 1), e, g, 9, dtype, periodic)


@pytest.mark.parametrize("periodic", [(True, False), (False, False)])
def test_cg_solves_variable_diffusion(grids, periodic):
    for dtype, rtol, cap in SOLVES:
        check_cg(grids[periodic], dtype, rtol, cap)


def test_gradient_is_the_adjoint(grids):
    offsets, shape = TAPSETS["asym4"], (2, 13, 14)
    st = grids[(True, False)].make_variable_stencil(
        shape, torch.float64, "cpu", offsets, int_coef(offsets, shape, 3))
    x = int_data(shape, torch.float64, 1).requires_grad_()
    g = int_data(shape, torch.float64, 2)
    st.apply_ad(x).backward(g)
    assert torch.equal(x.grad, st.adjoint(g))


def test_validation_refusals_and_set_coefficients(grids):
    grid = grids[(True, True)]
    shape, offs = (2, 9, 10), TAPSETS["star5"]
    coef = int_coef(offs, shape, 0)

    def make(offsets=offs, c=coef, **kw):
        return grid.make_variable_stencil(shape, torch.float32, "cpu",
                                          offsets, c, **kw)

    with pytest.raises(ValueError, match="duplicate"):
        make(offs[:4] + [offs[0]])
    for bad in ([(0, 0)], [(0, 5)] + offs[:4]):
        with pytest.raises(ValueError, match="radius"):
            make(bad, coef[:len(bad)])
    for bad in ([], [(dy, dx) for dy in (-1, 0, 1) for dx in range(-2, 3)]):
        with pytest.raises(ValueError, match="1..13 taps"):
            make(bad, torch.zeros(len(bad), 9, 10))
    for bad in (coef[:4], coef[:, :8], coef[0], coef[:, None]):
        with pytest.raises(ValueError, match="shape"):
            make(c=bad)
    with pytest.raises(TypeError, match="real"):
        make(c=coef.to(torch.complex64))
    with pytest.raises(ValueError, match="_levels_per_block"):
        make(_levels_per_block=3)
    st = make()
    for call in (st.gershgorin_bounds, lambda: st.make_chebyshev(1.0, 2.0)):
        with pytest.raises(TypeError, match="constant-coefficient only"):
            call()
    with pytest.raises(ValueError, match="shape"):
        st.set_coefficients(coef[:4])
    with pytest.raises(TypeError, match="real"):
        st.set_coefficients(coef.to(torch.complex64))
    x = int_data(shape, torch.float32, 4)
    before, ptr = st.apply(x), st.coefficients.data_ptr()
    st.set_coefficients(2 * coef)
    assert st.coefficients.data_ptr() == ptr
    assert torch.equal(st.apply(x), 2 * before) and before.any()
