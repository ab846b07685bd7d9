"""GPU suite for parallel/stencil.HaloStencil: the native executor
(csrc/stencil.hip + bridge.cpp:halo_stencil_nd / halo_stencil_adjoint_nd)
at world 1.

Periodic self-wraps cover the direct path (one launch, halo cells read
from the input field itself); ``_force_remote=True`` sends the same strips
to self through the RCCL group and covers the staged path (halo cells read
from the receive slots).  Oracles, data and the a-priori bound are those
of tests/test_halo_stencil.py.
"""

import itertools

import pytest
import torch

import mpi4jax_amd as m
from mpi4jax_amd.parallel.grid import CartesianGrid
from test_gpu_halo_exchanger import OPEN, SHAPES, _valid
from test_halo_adjoint import int_data, source_map
from test_halo_stencil import (KINDS, as_tuple, chain_gradients, check_bound,
                               gamma, interior, make_weights, ntaps,
                               oracle_apply, oracle_adjoint_chain, unit_acc,
                               unit_out)

pytestmark = pytest.mark.gpu

ALL = OPEN + [(False, False)]
DTYPES = (torch.float32, torch.float64, torch.bfloat16, torch.float16)
# several tiles in both axes plus a ragged edge (tiles are 32 x 64)
BIG = [(3, 41, 70), (2, 67, 131), (2, 76, 140)]
# n == 3 * width and 3 * width + 1 at width 4, and the larger two of BIG:
# (2, 67, 131) has a tile on the kernel's fast fill at width 1 only,
# (2, 76, 140) one at every width in both modes (test_fast_fill_is_reached)
MORE = [(12, 12), (13, 12), (2, 67, 131), (2, 76, 140)]
TILE_Y, TILE_X = 32, 64  # kStencilTileY, kStencilTileX of csrc/kernels.h


def fast_tiles(ny, nx, w, mode):
    """Tiles of an (ny, nx) plane that take halo_stencil_kernel's fast
    fill (the register-staged main[]/side[] loads): its `fast` condition,
    evaluated for every tile of the launch.  mode 0 = apply (outputs are
    the interior), 1 = adjoint (the full array)."""
    org = w if mode == 0 else 0
    oy, ox = (ny - 2 * w, nx - 2 * w) if mode == 0 else (ny, nx)
    rows, stride = TILE_Y + 2 * w, TILE_X + 2 * w
    n = 0
    for tiy in range(-(-oy // TILE_Y)):
        for tix in range(-(-ox // TILE_X)):
            fy0 = org + tiy * TILE_Y - w
            fx0 = org + tix * TILE_X - w
            n += (fy0 >= w and fx0 >= w and fy0 + rows <= ny - w
                  and fx0 + stride <= nx - w)
    return n


@pytest.fixture(scope="module", autouse=True)
def _init():
    m.init()
    yield
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def grids():
    return {p: CartesianGrid(dims=(1, 1), periodic=p) for p in ALL}


def _ext():
    from mpi4jax_amd._backend import rccl

    return rccl.ext()


def _cuda(ts):
    return [t.cuda() for t in ts]


def test_fast_fill_is_reached():
    """The shapes of MORE put at least one tile on the fast fill at every
    width in both modes (so the ten fill iterations of width 4 run), and
    the previous largest shape did so at width 1 only."""
    for w in (1, 2, 3, 4):
        for mode in (0, 1):
            assert fast_tiles(76, 140, w, mode) >= 1, (w, mode)
            assert (fast_tiles(67, 131, w, mode) >= 1) == (w == 1)
            assert (2, 76, 140) in MORE and _valid((2, 76, 140), w)


# ------------------------------------------------------------ direct path

@pytest.mark.parametrize("periodic", ALL)
@pytest.mark.parametrize("w", [1, 2, 3, 4])
def test_direct_path_matches_cpu_and_oracle(grids, periodic, w):
    """Bitwise on integer data, against the float64 oracle and against the
    CPU executor; the kinds of weights rotate over the cases."""
    grid = grids[periodic]
    ran = 0
    kinds = itertools.cycle(KINDS)
    for shape, nf in itertools.product(SHAPES + MORE, (1, 3, 8)):
        if not _valid(shape, w):
            continue
        k = make_weights(next(kinds), w, seed=nf)
        base = [int_data(shape, torch.float64, 7 * i + nf) for i in range(nf)]
        exp = oracle_apply(grid, k, base)
        for dtype in DTYPES:
            x = [b.to(dtype) for b in base]
            cpu = as_tuple(grid.make_stencil(shape, dtype, "cpu", k,
                                             nfields=nf).apply(*x))
            st = grid.make_stencil(shape, dtype, "cuda", k, nfields=nf)
            dev = _cuda(x)
            got = as_tuple(st.apply(*dev))
            for g, c, e, d, f in zip(got, cpu, exp, dev, x):
                g = g.cpu()
                assert torch.equal(d.cpu(), f), "apply() mutated its input"
                assert torch.equal(g, c), (shape, nf, dtype)
                assert torch.equal(interior(g, w).double(),
                                   e.to(dtype).double()), (shape, nf, dtype)
            ran += 1
    # widths 1..4 keep 10, 9, 5 and 2 of SHAPES, and all of MORE
    assert ran >= ({1: 10, 2: 9, 3: 5, 4: 2}[w] + 4) * 3 * 4


@pytest.mark.parametrize("periodic", ALL)
@pytest.mark.parametrize("w", [1, 2, 3, 4])
def test_direct_adjoint_matches_cpu_and_oracle(grids, periodic, w):
    grid = grids[periodic]
    ran = 0
    kinds = itertools.cycle(KINDS)
    for shape, nf in itertools.product(SHAPES + MORE, (1, 3)):
        if not _valid(shape, w):
            continue
        k = make_weights(next(kinds), w, seed=nf)
        src = source_map(grid, shape, w)
        for dtype in DTYPES:
            y = [int_data(shape, dtype, 5 * i + nf) for i in range(nf)]
            cpu = as_tuple(grid.make_stencil(shape, dtype, "cpu", k,
                                             nfields=nf).adjoint(*y))
            st = grid.make_stencil(shape, dtype, "cuda", k, nfields=nf)
            dev = _cuda(y)
            got = as_tuple(st.adjoint(*dev))
            for g, c, d, f in zip(got, cpu, dev, y):
                g = g.cpu()
                assert torch.equal(d.cpu(), f), "adjoint() mutated its input"
                assert torch.equal(g, c), (shape, nf, dtype)
                assert torch.equal(
                    g.double(), oracle_adjoint_chain(src, k, f, dtype)), \
                    (shape, nf, dtype)
            ran += 1
    assert ran >= ({1: 10, 2: 9, 3: 5, 4: 2}[w] + 4) * 2 * 4


# ------------------------------------------------------------ staged path

@pytest.mark.parametrize("periodic", OPEN)
@pytest.mark.parametrize("w", [1, 2, 4])
def test_staged_path_equals_direct_path_bitwise(grids, periodic, w):
    """Random normal data: the same arithmetic in the same order, only the
    halo reads differ.  apply and adjoint."""
    grid = grids[periodic]
    torch.manual_seed(11)
    k = torch.randn(2 * w + 1, 2 * w + 1, dtype=torch.float64)
    k[0, 1] = 0.0
    for shape, nf, dtype in itertools.product(
            SHAPES + BIG[:1], (1, 3), (torch.float32, torch.bfloat16)):
        if not _valid(shape, w):
            continue
        x = [torch.randn(shape, device="cuda").to(dtype) for _ in range(nf)]
        direct = grid.make_stencil(shape, dtype, "cuda", k, nfields=nf)
        staged = grid.make_stencil(shape, dtype, "cuda", k, nfields=nf,
                                   _force_remote=True)
        assert not staged.exchanger.local_directions
        keep = [f.clone() for f in x]
        for a, b in zip(as_tuple(staged.apply(*x)),
                        as_tuple(direct.apply(*x))):
            assert torch.equal(a, b), (shape, nf, dtype)
        for a, b in zip(as_tuple(staged.adjoint(*x)),
                        as_tuple(direct.adjoint(*x))):
            assert torch.equal(a, b), (shape, nf, dtype)
        for f, kp in zip(x, keep):
            assert torch.equal(f, kp), "the staged path wrote its input"


@pytest.mark.parametrize("force_remote", [False, True])
def test_staging_poison(grids, force_remote):
    """The direct path leaves staging alone and creates no communicator;
    the staged path reads only what it packed or received."""
    shape, w, nf = (2, 9, 10), 2, 3
    k = make_weights("asym", w)
    for periodic, dtype in itertools.product(
            OPEN, (torch.float32, torch.bfloat16)):
        grid = grids[periodic]
        x = [int_data(shape, dtype, i) for i in range(nf)]
        exp = oracle_apply(grid, k, x)
        st = grid.make_stencil(shape, dtype, "cuda", k, nfields=nf,
                               _force_remote=force_remote)
        ex = st.exchanger
        ex._sbuf.view(torch.uint8).fill_(0xFF)  # NaN pattern
        ex._rbuf.view(torch.uint8).fill_(0xFF)
        before = _ext().comm_count()
        dev = _cuda(x)
        got = as_tuple(st.apply(*dev))
        torch.cuda.synchronize()
        for g, e, d, f in zip(got, exp, dev, x):
            assert torch.equal(interior(g.cpu(), w).double(),
                               e.to(dtype).double())
            assert torch.equal(d.cpu(), f)
        if not force_remote:
            assert bool((ex._sbuf.view(torch.uint8) == 0xFF).all())
            assert bool((ex._rbuf.view(torch.uint8) == 0xFF).all())
            assert _ext().comm_count() == before
        # the adjoint reads no stale staging either
        src = source_map(grid, shape, w)
        ex._sbuf.view(torch.uint8).fill_(0xFF)
        ex._rbuf.view(torch.uint8).fill_(0xFF)
        for g, f in zip(as_tuple(st.adjoint(*dev)), x):
            assert torch.equal(g.cpu().double(),
                               oracle_adjoint_chain(src, k, f, dtype))


# ------------------------------------------------------------ random data

@pytest.mark.parametrize("shape", BIG)
@pytest.mark.parametrize("w", [1, 4])
def test_random_data_within_bound(grids, shape, w, monkeypatch):
    """apply and adjoint against the float64 oracle, native and Python
    executor on the GPU.

    The adjoint's bound, by the same reasoning as apply's: a term passes
    through at most n + 2 roundings in S^T (n adds, its product, its
    coefficient), the store of S^T, at most 9 adds in the exchange's
    adjoint and the final store.  With u_out the unit roundoff of a
    float16 / bfloat16 store (0 otherwise) every term is off by a factor
    within (1 + u)^(n + 11) (1 + u_out)^2, so
    ``|got - exact| <= (gamma(n + 11) (1 + u_out)^2 + 2 u_out + u_out^2)
    * mag`` with ``mag = E^T |S^T| |gout|``."""
    torch.manual_seed(13)
    k = torch.randn(2 * w + 1, 2 * w + 1, dtype=torch.float64)
    k[2 * w, 0] = 0.0
    n = ntaps(k)
    for periodic, dtype in itertools.product(
            ALL, (torch.float32, torch.float64, torch.bfloat16)):
        grid = grids[periodic]
        x = [torch.randn(shape).to(dtype) for _ in range(2)]
        exp, mag = oracle_apply(grid, k, x, with_mag=True)
        src = source_map(grid, shape, w)
        adj = [oracle_adjoint_chain(src, k, f, torch.float64, with_mag=True)
               for f in x]
        uo = unit_out(dtype)
        factor = (gamma(n + 11, unit_acc(dtype)) * (1 + uo) ** 2
                  + 2 * uo + uo * uo)
        st = grid.make_stencil(shape, dtype, "cuda", k, nfields=2)
        dev = _cuda(x)
        for env in (None, "1"):
            if env:
                monkeypatch.setenv("MPI4JAX_AMD_HALO_PY", env)
            else:
                monkeypatch.delenv("MPI4JAX_AMD_HALO_PY", raising=False)
            for o, e, g in zip(st.apply(*dev), exp, mag):
                check_bound(interior(o, w), e, g, n, dtype,
                            ("apply", env, periodic, dtype))
            for o, (e, g) in zip(st.adjoint(*dev), adj):
                err = (o.cpu().double() - e).abs()
                assert (err <= factor * g).all(), \
                    ("adjoint", env, periodic, dtype, err.max().item())
        monkeypatch.delenv("MPI4JAX_AMD_HALO_PY", raising=False)


def test_native_equals_python_executor_on_integer_data(grids, monkeypatch):
    shape, w, nf = (5, 11, 13), 2, 3
    for periodic, dtype in itertools.product(ALL, DTYPES):
        k = make_weights("full", w)
        st = grids[periodic].make_stencil(shape, dtype, "cuda", k,
                                          nfields=nf)
        x = [int_data(shape, dtype, i, "cuda") for i in range(nf)]
        monkeypatch.delenv("MPI4JAX_AMD_HALO_PY", raising=False)
        native = st.apply(*x) + st.adjoint(*x)
        monkeypatch.setenv("MPI4JAX_AMD_HALO_PY", "1")
        py = st.apply(*x) + st.adjoint(*x)
        monkeypatch.delenv("MPI4JAX_AMD_HALO_PY", raising=False)
        for a, b in zip(native, py):
            assert torch.equal(a, b), (periodic, dtype)


# ---------------------------------------------------------------- autodiff

def test_gradient_equals_cpu_on_integer_data(grids):
    shape, w = (2, 9, 10), 2
    for periodic, kind in itertools.product(ALL, ("star", "asym")):
        k = make_weights(kind, w)
        x = int_data(shape, torch.float64, 1)
        g = int_data(shape, torch.float64, 2)
        gpu, ref = chain_gradients(grids[periodic], k, x, g, device="cuda")
        cpu, _ = chain_gradients(grids[periodic], k, x, g)
        assert torch.equal(gpu, cpu) and torch.equal(gpu, ref), \
            (periodic, kind)
    # two fields, one of them requiring grad, float32
    st = {d: grids[(True, True)].make_stencil(
        shape, torch.float32, d, make_weights("asym", w), nfields=2)
        for d in ("cpu", "cuda")}
    grads = {}
    for d in ("cpu", "cuda"):
        a = int_data(shape, torch.float32, 3, d).requires_grad_()
        b = int_data(shape, torch.float32, 4, d)
        oa, ob = st[d].apply_ad(a, b)
        ref = st[d].apply(a.detach(), b)
        assert torch.equal(oa.detach(), ref[0])
        assert torch.equal(ob.detach(), ref[1])
        (oa * int_data(shape, torch.float32, 5, d)).sum().backward()
        assert b.grad is None
        grads[d] = a.grad.cpu()
    assert torch.equal(grads["cpu"], grads["cuda"])


def test_gradcheck_on_gpu(grids):
    torch.manual_seed(22)
    k = torch.randn(5, 5, dtype=torch.float64)
    st = grids[(True, True)].make_stencil(
        (2, 6, 7), torch.float64, "cuda", k, nfields=2)
    a = torch.randn(2, 6, 7, dtype=torch.float64, device="cuda",
                    requires_grad=True)
    b = torch.randn(2, 6, 7, dtype=torch.float64, device="cuda")
    assert torch.autograd.gradcheck(lambda x: st.apply_ad(x, b), (a,))


# ------------------------------------------------------------- large sizes

def test_more_than_65535_planes(grids):
    shape, w = (70000, 3, 3), 1
    k = make_weights("asym", w)
    for periodic in ((True, True), (True, False)):
        grid = grids[periodic]
        x = int_data(shape, torch.float32, 9)
        st = grid.make_stencil(shape, torch.float32, "cuda", k)
        got = st.apply(x.cuda()).cpu()
        (exp,) = oracle_apply(grid, k, [x])
        assert torch.equal(interior(got, w).double(), exp)
        src = source_map(grid, shape, w)
        gin = st.adjoint(x.cuda()).cpu()
        assert torch.equal(gin.double(),
                           oracle_adjoint_chain(src, k, x, torch.float32))


def test_offsets_past_2_31():
    """float16 (1, 46400, 46400), width 1, periodic, three taps:
    out[j, i] = 2 v[j-1, i] - v[j, i+1] + 3 v[j+1, i-1] with v the wrapped
    field.  The data is zero off a few rows and columns at both ends and
    mid-field; sums stay below 18, exact in float16.  Past 2^31 elements
    lie the north rows and the high ends of the columns."""
    ny = nx = 46400
    grid = CartesianGrid(dims=(1, 1), periodic=(True, True))
    k = [[0.0, 2.0, 0.0], [0.0, 0.0, -1.0], [3.0, 0.0, 0.0]]
    f = u = out = st = pre = None
    try:
        f = torch.zeros(1, ny, nx, dtype=torch.float16, device="cuda")
        assert f.numel() > 1 << 31
        u = f[0]
        ramp = torch.arange(nx, device="cuda")
        mid = ny // 2
        lines = (0, 1, 2, 3, ny - 4, ny - 3, ny - 2, ny - 1,
                 mid - 1, mid, mid + 1)
        for n_, j in enumerate(lines):
            u[j] = ((ramp * (n_ + 2)) % 7 - 3).to(torch.float16)
        for n_, i in enumerate(lines[:8]):
            u[:, i] = ((ramp * (n_ + 3)) % 5 - 2).to(torch.float16)
        pre = {j: u[j].clone() for j in lines}
        st = grid.make_stencil(f.shape, f.dtype, "cuda", k)
        out = st.apply(f)[0]
        for j in lines:
            assert torch.equal(u[j], pre[j]), "apply() mutated its input"

        def wrap(line):  # halo ends of a row or a column of v
            line = line.clone()
            line[0] = line[-2]
            line[-1] = line[1]
            return line

        def vrow(j):
            return wrap(u[ny - 2 if j == 0 else 1 if j == ny - 1 else j])

        def vcol(i):
            return wrap(u[:, nx - 2 if i == 0 else 1 if i == nx - 1 else i])

        for j in (1, 2, ny - 3, ny - 2, mid):
            exp = (2 * vrow(j - 1)[1:-1] - vrow(j)[2:]
                   + 3 * vrow(j + 1)[:-2])
            assert torch.equal(out[j, 1:-1], exp), j
            assert int(torch.count_nonzero(exp)) > 0
        for i in (1, 2, nx - 3, nx - 2):
            exp = (2 * vcol(i)[:-2] - vcol(i + 1)[1:-1]
                   + 3 * vcol(i - 1)[2:])
            assert torch.equal(out[1:-1, i], exp), i
        # the halo of a fresh output stays zero, the input is unchanged
        for halo in (out[0], out[ny - 1], out[:, 0], out[:, nx - 1]):
            assert int(torch.count_nonzero(halo)) == 0
        assert int(torch.count_nonzero(u[5])) == 8
    finally:
        del f, u, out, st, pre
        torch.cuda.empty_cache()


# ------------------------------------------------------ capture, validation

def test_graph_capture_and_no_allocation(grids):
    shape, w, nf = (3, 41, 70), 2, 3
    grid = grids[(True, True)]
    k = make_weights("star", w)
    st = grid.make_stencil(shape, torch.float32, "cuda", k, nfields=nf)
    torch.manual_seed(9)
    x = [torch.randn(shape, device="cuda") for _ in range(nf)]
    o = [torch.zeros(shape, device="cuda") for _ in range(nf)]
    gi = [torch.zeros(shape, device="cuda") for _ in range(nf)]

    def run():
        st.apply(*x, out=o)
        st.adjoint(*x, out=gi)

    run()  # warm-up
    torch.cuda.synchronize()
    n0 = torch.cuda.memory_stats()["allocation.all.allocated"]
    run()
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == n0, \
        "apply / adjoint with out= allocated after warm-up"

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()

    fresh = [torch.randn(shape, device="cuda") for _ in range(nf)]
    eager = grid.make_stencil(shape, torch.float32, "cuda", k, nfields=nf)
    e_out = eager.apply(*fresh)
    e_gin = eager.adjoint(*fresh)
    for f, n_ in zip(x, fresh):
        f.copy_(n_)
    for t in o + gi:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(o + gi, e_out + e_gin):
        assert torch.equal(a, b)
        assert a.abs().max() > 0


def test_native_entries_validate(grids):
    """Both pybind entries check every argument themselves and raise
    before anything is enqueued.  The block-count limit has a test of its
    own below; the 2^31 limit on extents cannot be reached by tensors
    that fit in memory."""
    ext = _ext()
    f = torch.ones(2, 9, 10, device="cuda")
    o = torch.full((2, 9, 10), 7.0, device="cuda")
    pair = torch.ones(2, 2, 9, 10, device="cuda")
    buf = torch.zeros(4096, device="cuda")
    none = [-1] * 8
    wrap = [0, 0] + [-1] * 6
    names = ("fields", "outs", "levels", "ny", "nx", "width", "tap_dy",
             "tap_dx", "tap_coef", "send_to", "recv_from", "local_mask",
             "sbuf", "rbuf", "comm_id")
    ok = ([f], [o], 2, 9, 10, 2, [0, -2, 2], [0, 2, -1], [1.0, 2.0, 3.0],
          wrap, wrap, 0b11, buf, buf.clone(), -1)
    fi = torch.ones(2, 9, 10, dtype=torch.int32, device="cuda")
    oi = torch.full((2, 9, 10), 7, dtype=torch.int32, device="cuda")
    bi = torch.zeros(4096, dtype=torch.int32, device="cuda")
    bad_args = (
        dict(fields=[], outs=[]), dict(fields=[f] * 9, outs=[o] * 9),
        dict(width=0), dict(width=4), dict(ny=10), dict(levels=3),
        dict(send_to=none[:7]), dict(local_mask=256),
        dict(local_mask=0b100), dict(sbuf=buf[:8]),
        dict(rbuf=buf.double()), dict(sbuf=buf.cpu()),
        dict(fields=[f.cpu()]), dict(fields=[f.transpose(1, 2)]),
        dict(send_to=[-2] + none[1:], local_mask=0),
        # the stencil's own
        dict(tap_dy=[], tap_dx=[], tap_coef=[]),
        dict(tap_dy=[0] * 82, tap_dx=[0] * 82, tap_coef=[1.0] * 82),
        dict(tap_dy=[0, 1]), dict(tap_dx=[0, 1]), dict(tap_coef=[1.0]),
        dict(tap_dy=[0, 3, 2]), dict(tap_dx=[0, 2, -3]),
        dict(fields=[fi], outs=[oi], sbuf=bi, rbuf=bi.clone()),
        dict(outs=[]), dict(outs=[o, o.clone()]),
        dict(outs=[torch.zeros(2, 9, 11, device="cuda")]),
        dict(outs=[torch.zeros(2, 10, 9, device="cuda")]),
        dict(outs=[o.double()]), dict(outs=[o.cpu()]),
        dict(outs=[torch.zeros(2, 9, 20, device="cuda")[..., ::2]]),
        dict(outs=[f]),  # output is the input
        dict(fields=[pair[0], pair[1]], outs=[o, pair[1]]),
        dict(fields=[pair[0], pair[1]], outs=[o, o]),
        # an output that starts inside input 0
        dict(fields=[pair[0], f],
             outs=[o, pair.view(-1)[90:270].view(2, 9, 10)]),
        # a comm that does not exist, on a call with a remote entry
        dict(local_mask=0, comm_id=123456),
    )
    for entry in (ext.halo_stencil_nd, ext.halo_stencil_adjoint_nd):
        def call(**kw):
            args = dict(zip(names, ok))
            args.update(kw)
            entry(*(args[n] for n in names))

        call()
        torch.cuda.synchronize()
        assert not torch.equal(o, torch.full_like(o, 7.0))
        o.fill_(7.0)
        for bad in bad_args:
            with pytest.raises((RuntimeError, ValueError)):
                call(**bad)
        # width 5 on a field large enough for it
        f5 = torch.ones(1, 15, 16, device="cuda")
        with pytest.raises((RuntimeError, ValueError)):
            entry([f5], [torch.zeros_like(f5)], 1, 15, 16, 5, [0], [0],
                  [1.0], wrap, wrap, 0b11, buf, buf.clone(), -1)
        torch.cuda.synchronize()
        assert torch.equal(o, torch.full_like(o, 7.0))
        assert torch.equal(oi, torch.full_like(oi, 7))
        assert torch.equal(f, torch.ones_like(f))
        assert torch.equal(pair, torch.ones_like(pair))


def test_block_count_limit(grids):
    """A launch holds fewer than 2^32 threads, that is fewer than 2^24
    blocks of 256.  (n, 3, 3) at width 1 is one block per plane in both
    modes: 2^24 - 1 planes are the largest grid and must compute, 2^24
    planes must raise ValueError from both entries before anything is
    enqueued.  The staging of such a field (12 elements per plane) stays
    far below its own 2^31 limit."""
    n = 1 << 24
    grid = grids[(True, True)]
    k = [[0.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 3.0]]
    x = o = st = big = None
    try:
        x = torch.ones(n, 3, 3, device="cuda")
        x[:, 1, 1] = torch.arange(n, device="cuda") % 5 - 2.0
        o = torch.full((n, 3, 3), 7.0, device="cuda")
        # one plane short of the limit: the last block of the largest grid
        st = grid.make_stencil((n - 1, 3, 3), torch.float32, "cuda", k)
        st.apply(x[:n - 1], out=o[:n - 1])
        # the one interior cell is its own neighbour in every direction
        assert torch.equal(o[:n - 1, 1, 1], 5.0 * x[:n - 1, 1, 1])
        o[:n - 1, 1, 1] = 7.0
        assert bool((o == 7.0).all())
        st.adjoint(x[:n - 1], out=o[:n - 1])
        assert torch.equal(o[:n - 1, 1, 1], 5.0 * x[:n - 1, 1, 1])
        assert int(torch.count_nonzero(o[:n - 1, 0])) == 0
        assert bool((o[n - 1] == 7.0).all())
        o.fill_(7.0)
        st = None  # frees its staging
        big = grid.make_stencil((n, 3, 3), torch.float32, "cuda", k)
        for fn in (big.apply, big.adjoint):
            with pytest.raises(ValueError, match="2\\^24"):
                fn(x, out=o)
        ex = big.exchanger
        for entry in (_ext().halo_stencil_nd,
                      _ext().halo_stencil_adjoint_nd):
            with pytest.raises(ValueError, match="2\\^24"):
                entry([x], [o], n, 3, 3, 1, [0, 1], [0, 1], [2.0, 3.0],
                      ex._send_to, ex._recv_from, ex._local_mask, ex._sbuf,
                      ex._rbuf, -1)
        torch.cuda.synchronize()
        assert bool((o == 7.0).all())
    finally:
        del x, o, st, big
        torch.cuda.empty_cache()
