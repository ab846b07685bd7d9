"""CPU suite for parallel/stencil3d.HaloStencil3D
(``CartesianGrid.make_stencil3d``), and the helpers it shares with
tests/test_gpu_stencil3d.py.

Oracle: ``HaloExchanger.exchange`` of the fields in float64 on the CPU,
padded with zeros (or wrapped) along z, then ``sum_t K_t * shifted slice``
in float64.  Integer fields in [-4, 4] with integer weights in [-2, 2] keep
every partial sum of at most 27 taps within 216, exact in every dtype, so
those results are compared bitwise.
"""

import itertools
import math

import pytest
import torch
import torch.nn.functional as F

import mpi4jax_amd as m
from mpi4jax_amd.parallel import HaloStencil3D
from mpi4jax_amd.parallel.grid import CartesianGrid
from _mp import run_multiproc
from test_halo_adjoint import int_data
from test_halo_exchanger import DIMS, PERIODIC, fake_grid
from test_halo_stencil import as_tuple, interior
from test_stencil_cg import int_dot

DTYPES = (torch.float64, torch.float32, torch.bfloat16, torch.float16)
ZB = ("zero", "periodic")


def int_weights(rz, r, seed, keep=None):
    """Integer weights in [-2, 2] \\ {0} on the offsets ``keep`` accepts."""
    g = torch.Generator().manual_seed(seed)
    n = (2 * rz + 1, 2 * r + 1, 2 * r + 1)
    k = torch.randint(1, 3, n, generator=g).double()
    k *= torch.randint(0, 2, n, generator=g).double() * 2 - 1
    for a, b, c in itertools.product(*map(range, n)):
        if keep and not keep(a - rz, b - r, c - r):
            k[a, b, c] = 0.0
    return k


def _star(dz, dy, dx):
    return (dz != 0) + (dy != 0) + (dx != 0) <= 1


TAPSETS = {
    "star7": int_weights(1, 1, 1, _star),
    "box27": int_weights(1, 1, 2),
    "star13": int_weights(2, 2, 3, _star),
    "asym4": int_weights(1, 3, 4, lambda *o: o in (
        (-1, 3, -1), (0, 0, 2), (1, -3, 0), (1, 1, 3))),
    "flat": int_weights(0, 2, 5, lambda dz, dy, dx: (dy + dx) % 2 == 0),
    "star19": int_weights(1, 4, 6, _star),  # r = 4: the largest LDS tile
}
LAP7 = torch.zeros(3, 3, 3, dtype=torch.float64)
for _o in ((0, 1, 1), (2, 1, 1), (1, 0, 1), (1, 2, 1), (1, 1, 0), (1, 1, 2)):
    LAP7[_o] = -1.0
LAP7[1, 1, 1] = 7.0  # I - lap7, nu = 1
SOLVES = [(torch.float64, 1e-10), (torch.float32, 1e-5)]


def oracle(grid, weights, fields, zb, with_mag=False):
    """Interior of ``A`` on ``fields`` in float64 (and ``sum |K| |v|``)."""
    rz, w = (weights.shape[0] - 1) // 2, (weights.shape[1] - 1) // 2
    shape = tuple(fields[0].shape)
    nz, ny, nx = shape[-3:]
    ex = grid.make_halo_exchanger(shape, torch.float64, "cpu", width=w,
                                  nfields=len(fields))
    outs, mags = [], []
    for v in as_tuple(ex.exchange(*(f.detach().cpu().double()
                                    for f in fields))):
        v = v.reshape(-1, nz, ny, nx)
        v = (torch.cat([v[:, nz - rz:], v, v[:, :rz]], 1) if zb == "periodic"
             else F.pad(v, (0, 0, 0, 0, rz, rz)))
        out = torch.zeros(v.shape[0], nz, ny - 2 * w, nx - 2 * w,
                          dtype=torch.float64)
        mag = torch.zeros_like(out)
        for a, b, c in itertools.product(*map(range, weights.shape)):
            s = v[:, a:a + nz, b:ny - 2 * w + b, c:nx - 2 * w + c]
            out += weights[a, b, c] * s
            mag += weights[a, b, c].abs() * s.abs()
        outs.append(out.reshape(shape[:-2] + out.shape[-2:]))
        mags.append(mag.reshape(outs[-1].shape))
    return (outs, mags) if with_mag else outs


def cg_cap(rtol, kappa=13.0):
    """CG's a-priori iteration bound for condition number ``kappa``
    (Gershgorin: 1 <= lambda(I - lap7) <= 13)."""
    s = math.sqrt(kappa)
    return math.ceil(math.log(2 * s / rtol) / math.log((s + 1) / (s - 1)))


def check_cg(grid, dtype, rtol, cap, device="cpu"):
    """The acceptance of tests/test_stencil_cg.py::test_solve_table on
    ``(I - lap7) x = b``, shape (4, 12, 14), zero z boundary, with the true
    residual recomputed by the float64 oracle."""
    g = torch.Generator().manual_seed(5)
    b = F.pad(torch.randn(4, 10, 12, generator=g, dtype=torch.float64),
              (1, 1, 1, 1)).to(dtype).to(device)
    st = grid.make_stencil3d(b.shape, dtype, device, LAP7)
    assert st.gershgorin_bounds() == (1.0, 13.0)
    x, info = st.make_cg().solve(b, rtol=rtol, maxiter=cap, check_every=1)
    assert info.converged is True and info.iterations <= cap
    assert info.residual_norm <= rtol * info.rhs_norm
    (ax,) = oracle(grid, LAP7, [x], "zero")
    bi = interior(b.cpu().double(), 1)
    true = ((bi - ax).norm() / bi.norm()).item()
    assert true <= 2 * rtol, (dtype, true)
    return st, b, x, info.iterations


@pytest.fixture(scope="module")
def grids():
    m.init()
    return {p: CartesianGrid(dims=(1, 1), periodic=p) for p in PERIODIC}


@pytest.mark.parametrize("zb", ZB)
@pytest.mark.parametrize("periodic", PERIODIC)
@pytest.mark.parametrize("name", list(TAPSETS))
def test_apply_exact_and_adjoint_identity(grids, periodic, name, zb):
    grid, k = grids[periodic], TAPSETS[name]
    rz, w = (k.shape[0] - 1) // 2, (k.shape[1] - 1) // 2
    for shape, nf in itertools.product(
            [(2 * rz + 1, 3 * w, 3 * w + 1), (2, 5, 13, 14)], (1, 3)):
        base = [int_data(shape, torch.float64, 7 * i + nf) for i in range(nf)]
        exp = oracle(grid, k, base, zb)
        for dtype in DTYPES:
            st = grid.make_stencil3d(shape, dtype, "cpu", k, nfields=nf,
                                     z_boundary=zb)
            assert isinstance(st, HaloStencil3D)
            assert (st.width, st.z_radius, st.z_chunk) == (w, rz, 1)
            assert st.taps == [
                (a - rz, b - w, c - w, k[a, b, c].item())
                for a, b, c in itertools.product(*map(range, k.shape))
                if k[a, b, c] != 0]
            x = [f.to(dtype) for f in base]
            got = as_tuple(st.apply(*x))
            for o, e, f, s in zip(got, exp, x, base):
                assert torch.equal(f.double(), s), "apply() mutated its input"
                assert torch.equal(interior(o, w).double(), e), (shape, dtype)
            y = [int_data(shape, dtype, 50 + i) for i in range(nf)]
            gin = as_tuple(st.adjoint(*y))
            if dtype in (torch.float32, torch.float64):
                assert (sum(int_dot(a, b) for a, b in zip(got, y))
                        == sum(int_dot(a, b) for a, b in zip(x, gin)))


def test_zero_boundary_forms_no_tap_outside(grids):
    """nz = 1: every z tap drops out and the centre plane of the table is
    left."""
    k = TAPSETS["box27"]
    x = int_data((1, 6, 7), torch.float32, 3)
    st = grids[(True, True)].make_stencil3d(x.shape, torch.float32, "cpu", k)
    flat = grids[(True, True)].make_stencil(x.shape, torch.float32, "cpu",
                                            k[1])
    assert torch.equal(st.apply(x), flat.apply(x))
    assert torch.equal(st.adjoint(x), flat.adjoint(x))


def test_validation_refusals(grids):
    grid = grids[(True, True)]

    def make(k=TAPSETS["star7"], shape=(4, 9, 10), **kw):
        return grid.make_stencil3d(shape, torch.float32, "cpu", k, **kw)

    for bad in (torch.ones(3, 3), torch.ones(3, 2, 2), torch.ones(2, 3, 3),
                torch.ones(3, 3, 5)):
        with pytest.raises(ValueError, match="table"):
            make(bad)
    with pytest.raises(ValueError, match="z radius"):
        make(torch.ones(7, 3, 3))
    with pytest.raises(ValueError, match="radius"):
        make(torch.ones(1, 11, 11))
    with pytest.raises(ValueError, match="1..32 non-zero"):
        make(torch.ones(3, 5, 5))
    with pytest.raises(ValueError, match="non-zero"):
        make(torch.zeros(3, 3, 3))
    with pytest.raises(ValueError, match="nz, ny, nx"):
        make(shape=(9, 10))
    with pytest.raises(ValueError, match="periodic z needs"):
        make(TAPSETS["star13"], z_boundary="periodic")
    with pytest.raises(ValueError, match="z_boundary"):
        make(z_boundary="reflect")
    for bad in (0, 5, True, 2.0):
        with pytest.raises(ValueError, match="_z_chunk"):
            make(_z_chunk=bad)
    assert make(_z_chunk=3).z_chunk == 3
    with pytest.raises(TypeError, match="no Chebyshev kernel"):
        make().make_chebyshev(1.0, 2.0)
    with pytest.raises(TypeError, match="float32 and float64"):
        grid.make_stencil3d((4, 9, 10), torch.float16, "cpu",
                            TAPSETS["star7"]).make_cg()


@pytest.mark.parametrize("dtype,rtol", SOLVES)
def test_cg_solves_3d(grids, dtype, rtol):
    check_cg(grids[(False, False)], dtype, rtol, cg_cap(rtol))


def test_gradient_is_the_adjoint(grids):
    st = grids[(True, False)].make_stencil3d(
        (3, 9, 10), torch.float64, "cpu", TAPSETS["asym4"],
        z_boundary="periodic")
    x = int_data((3, 9, 10), torch.float64, 1).requires_grad_()
    g = int_data((3, 9, 10), torch.float64, 2)
    st.apply_ad(x).backward(g)
    assert torch.equal(x.grad, st.adjoint(g))


# ---------------------------------------------------------------- world 2

BY, BX = 6, 8  # block of interior cells per rank


def _multirank(rank, ws):
    comm = m.get_world()
    dtype, k, w = torch.float64, TAPSETS["box27"], 1
    for dims, periodic, zb in itertools.product(DIMS[ws], PERIODIC, ZB):
        grid = CartesianGrid(comm=comm, dims=dims, periodic=periodic)
        one = fake_grid(0, (1, 1), periodic)
        cy, cx = grid.coords

        def block(t):
            return t[..., cy * BY:(cy + 1) * BY, cx * BX:(cx + 1) * BX]

        def local(t):
            return F.pad(block(t), (w, w, w, w)).contiguous()

        shape = (2, 3, BY * dims[0], BX * dims[1])
        G, Y = int_data(shape, dtype, 40), int_data(shape, dtype, 50)
        x, y = local(G), local(Y)
        G, Y = F.pad(G, (w, w, w, w)), F.pad(Y, (w, w, w, w))
        st = grid.make_stencil3d(x.shape, dtype, "cpu", k, z_boundary=zb)
        st1 = one.make_stencil3d(G.shape, dtype, "cpu", k, z_boundary=zb)
        what = (dims, periodic, zb, rank)
        assert torch.equal(interior(st.apply(x), w),
                           block(interior(st1.apply(G), w))), what
        assert torch.equal(interior(st.adjoint(y), w),
                           block(interior(st1.adjoint(Y), w))), what


def test_multirank_apply_and_adjoint():
    run_multiproc(_multirank, 2)
