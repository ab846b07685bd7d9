"""GPU suite for the Krylov layer over HaloStencil: the native executor
(csrc/krylov.hip, the DOT epilogue of csrc/stencil.hip and the four
bridge.cpp entries halo_stencil_dot_nd, halo_interior_dot_nd,
halo_cg_update_nd, halo_cg_direction_nd) at world 1.

Oracles, data and the SPD system are those of tests/test_stencil_cg.py.
Integer data makes every inner product exact, so native results are
compared bitwise with integer arithmetic and with the Python executor;
random data is held to the a-priori bound of ``test_random_dot_bound``,
which holds for any order of additions.
"""

import itertools
import math

import pytest
import torch

import mpi4jax_amd as m
from mpi4jax_amd.parallel.grid import CartesianGrid
from test_gpu_halo_exchanger import OPEN, _valid
from test_halo_adjoint import int_data
from test_halo_stencil import (as_tuple, gamma, interior, make_weights,
                               oracle_apply)
from test_stencil_cg import (SOLVES, SPD_PERIODIC, check_exact_dots,
                             check_exact_iteration, int_dot, spd_rhs,
                             spd_weights, true_residual)

pytestmark = pytest.mark.gpu

ALL = OPEN + [(False, False)]
DTYPES = (torch.float32, torch.float64, torch.bfloat16, torch.float16)
# n == 3 * width and 3 * width + 1 at width 4; batch dims; several 32 x 64
# tiles with ragged edges; and the one shape with a tile on the stencil
# kernel's fast fill at every width, so DOT runs after both fills
CG_SHAPES = [(12, 12), (13, 12), (2, 9, 10), (3, 41, 70), (2, 76, 140)]
U = 2.0 ** -53


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


def _poison(*tensors):
    for t in tensors:
        t.reshape(-1).view(torch.uint8).fill_(0xFF)  # NaN pattern


def _geom(st):
    ex = st.exchanger
    return ex.levels, ex.ny, ex.nx, st.width


# ------------------------------------------------- integer data, bitwise

@pytest.mark.parametrize("periodic", ALL)
@pytest.mark.parametrize("w", [1, 2, 3, 4])
def test_dots_native_python_and_oracle_agree(grids, periodic, w,
                                             monkeypatch):
    grid = grids[periodic]
    ran = 0
    for shape, nf, dtype in itertools.product(CG_SHAPES, (1, 3, 8), DTYPES):
        if not _valid(shape, w):
            continue
        monkeypatch.delenv("MPI4JAX_AMD_HALO_PY", raising=False)
        st, x, y, ref, want_xy, want_pap = check_exact_dots(
            grid, shape, w, nf, dtype, device="cuda")
        # the partials buffer is per stencil and was allocated once
        buf = st._partials_buf()
        assert st._partials_buf() is buf
        monkeypatch.setenv("MPI4JAX_AMD_HALO_PY", "1")
        assert st.dot(x, y).item() == want_xy
        out, pap = st.apply_dot(*x)
        assert pap.item() == want_pap
        for o, r in zip(as_tuple(out), ref):
            assert torch.equal(o, r)
        monkeypatch.delenv("MPI4JAX_AMD_HALO_PY", raising=False)
        ran += 1
    assert ran >= (5 if w < 4 else 4) * 3 * 4


@pytest.mark.parametrize("periodic", ALL)
def test_one_iteration_native_python_and_fractions_agree(grids, periodic,
                                                         monkeypatch):
    """Both executors against exact rational arithmetic, hence bitwise
    against each other."""
    cases = [((12, 12), 4, 3), ((13, 12), 4, 1), ((2, 9, 10), 1, 3),
             ((2, 9, 10), 2, 2), ((3, 41, 70), 3, 2), ((2, 76, 140), 1, 1),
             ((2, 76, 140), 4, 1)]
    for (shape, w, nf), dtype in itertools.product(
            cases, (torch.float32, torch.float64)):
        # the Python executor on the small shapes only: rational
        # arithmetic on the two large ones takes a second per run
        for env in (None, "1") if shape[-1] < 64 else (None,):
            if env:
                monkeypatch.setenv("MPI4JAX_AMD_HALO_PY", env)
            else:
                monkeypatch.delenv("MPI4JAX_AMD_HALO_PY", raising=False)
            check_exact_iteration(grids[periodic], shape, w, nf, dtype,
                                  device="cuda")
        monkeypatch.delenv("MPI4JAX_AMD_HALO_PY", raising=False)


# ------------------------------------------------------------ random data

@pytest.mark.parametrize("w", [1, 2, 4])
def test_apply_dot_output_is_applys_on_random_data(grids, w):
    torch.manual_seed(31)
    k = torch.randn(2 * w + 1, 2 * w + 1, dtype=torch.float64)
    k[0, 1] = 0.0
    for periodic, shape, dtype in itertools.product(ALL, CG_SHAPES, DTYPES):
        if not _valid(shape, w):
            continue
        x = [torch.randn(shape, device="cuda").to(dtype) for _ in range(2)]
        st = grids[periodic].make_stencil(shape, dtype, "cuda", k, nfields=2)
        ref = st.apply(*x)
        out, _ = st.apply_dot(*x)
        for o, r in zip(out, ref):
            assert torch.equal(o, r), (periodic, shape, dtype)


def _fsum_dot(a, b, w):
    """(correctly rounded sum, sum of magnitudes, cells) of the float64
    products of the interiors."""
    prods = []
    for fa, fb in zip(a, b):
        p = interior(fa.cpu().double(), w) * interior(fb.cpu().double(), w)
        prods += p.reshape(-1).tolist()
    return math.fsum(prods), math.fsum(abs(p) for p in prods), len(prods)


@pytest.mark.parametrize("shape", CG_SHAPES[2:])
def test_random_dot_bound(grids, shape):
    """The data is float32-valued (also in the float64 fields; values of
    the 16-bit types are), so every product of ``dot`` is exact in float64
    and ``math.fsum`` of the products is the correctly rounded exact sum.
    N float64 additions in any order then give
    ``|got - exact| <= gamma(N, 2^-53) * sum|a_i b_i| + 2^-53 |exact|``,
    the last term for the oracle's own rounding.  ``apply_dot`` multiplies
    by the stored output; in float64 fields that product is rounded once
    (or fused), in the kernel and in the oracle, which makes it
    ``gamma(N + 1) + 2^-53``."""
    torch.manual_seed(17)
    w = 2
    k = torch.randn(5, 5, dtype=torch.float64)
    for periodic, dtype in itertools.product(ALL, DTYPES):
        a = [torch.randn(shape).to(dtype).cuda() for _ in range(2)]
        b = [torch.randn(shape).to(dtype).cuda() for _ in range(2)]
        st = grids[periodic].make_stencil(shape, dtype, "cuda", k, nfields=2)
        for p, q in ((a, b), (a, a)):
            exact, mag, n = _fsum_dot(p, q, w)
            got = st.dot(p, q).item()
            assert abs(got - exact) <= gamma(n, U) * mag + U * abs(exact), \
                (periodic, dtype, got, exact)
        out, pap = st.apply_dot(*a)
        exact, mag, n = _fsum_dot(a, out, w)
        extra = dtype == torch.float64
        bound = ((gamma(n + extra, U) + extra * U) * mag + U * abs(exact))
        assert abs(pap.item() - exact) <= bound, (periodic, dtype)


# ------------------------------------------------- staged path, poisoning

@pytest.mark.parametrize("periodic", OPEN)
def test_staged_path_equals_direct_path_bitwise(grids, periodic):
    """``_force_remote`` sends the strips to self through the RCCL group
    and the scalars through a one-rank allreduce; the arithmetic is the
    same.  The direct path creates no communicator."""
    grid = grids[periodic]
    torch.manual_seed(5)
    for (shape, w), dtype in itertools.product(
            [((2, 9, 10), 2), ((3, 41, 70), 1), ((3, 41, 70), 4)],
            (torch.float32, torch.float64)):
        if w <= 2:
            k = spd_weights(w)
        else:  # symmetric and diagonally dominant
            k = 0.01 * torch.randn(9, 9, dtype=torch.float64)
            k = k + k.flip(0, 1)
            k[4, 4] = 1.0
        b = [torch.randn(shape, dtype=dtype, device="cuda")
             for _ in range(2)]
        res = {}
        for name in ("direct", "staged"):
            before = _ext().comm_count()
            st = grid.make_stencil(shape, dtype, "cuda", k, nfields=2,
                                   _force_remote=name == "staged")
            cg = st.make_cg()
            x = [torch.zeros_like(t) for t in b]
            cg.start(b, x)
            first = cg.rs.clone()
            cg.apply_step()
            pq = cg.pq.clone()
            cg.update_step()
            cg.direction_step()
            cg.iterate(2)
            out, pap = st.apply_dot(*b)
            res[name] = ([first, pq, cg.rs.clone(), cg.rs_old.clone(), pap]
                         + x + list(out) + list(cg.residual)
                         + list(cg.direction))
            if name == "direct":
                torch.cuda.synchronize()
                assert _ext().comm_count() == before, \
                    "the direct path created a communicator"
            else:
                assert not st.exchanger.local_directions
        for a, c in zip(res["direct"], res["staged"]):
            assert torch.equal(a, c), (shape, w, dtype)
            assert torch.isfinite(a).all()
    # bfloat16 apply_dot through the staged path
    k = make_weights("asym", 2)
    x = [int_data((2, 9, 10), torch.bfloat16, i, "cuda") for i in range(3)]
    got = [grid.make_stencil((2, 9, 10), torch.bfloat16, "cuda", k,
                             nfields=3, _force_remote=fr).apply_dot(*x)
           for fr in (False, True)]
    assert got[0][1].item() == got[1][1].item()
    for a, c in zip(got[0][0], got[1][0]):
        assert torch.equal(a, c)


def test_poisoned_partials_and_scalars(grids):
    """Every slot an entry reads was written by the same call: a NaN
    pattern in the partials buffer and in the scalar outputs changes
    nothing."""
    ext = _ext()
    for periodic, (shape, w), dtype in itertools.product(
            ALL, [((2, 9, 10), 2), ((3, 41, 70), 1)],
            (torch.float32, torch.float64)):
        grid = grids[periodic]
        k = make_weights("star", w, seed=2)
        st = grid.make_stencil(shape, dtype, "cuda", k, nfields=2)
        ex = st.exchanger
        a = [int_data(shape, dtype, 3 + i, "cuda") for i in range(2)]
        b = [int_data(shape, dtype, 8 + i, "cuda") for i in range(2)]
        part = st._partials_buf()
        # more slots than blocks: the tail must not be read either
        wide = torch.empty(part.numel() + 300, dtype=torch.float64,
                           device="cuda")
        res = torch.empty((), dtype=torch.float64, device="cuda")
        want = sum(int_dot(interior(p, w), interior(q, w))
                   for p, q in zip(a, b))
        for buf in (part, wide):
            _poison(buf, res)
            ext.halo_interior_dot_nd(a, b, *_geom(st), buf, res)
            assert res.item() == want
        outs = [torch.zeros_like(t) for t in a]
        exp = oracle_apply(grid, k, a)
        want = sum(int_dot(interior(p, w), e) for p, e in zip(a, exp))
        for buf in (part, wide):
            _poison(buf, res)
            ext.halo_stencil_dot_nd(
                a, outs, ex.levels, ex.ny, ex.nx, w, st._tap_dy, st._tap_dx,
                st._tap_coef, ex._send_to, ex._recv_from, ex._local_mask,
                ex._sbuf, ex._rbuf, -1, buf, res)
            assert res.item() == want
        # update: rs and pq are inputs, rs_old and the partials outputs
        ref = None
        for buf in (None, part, wide):
            x = [torch.zeros_like(t) for t in a]
            r = [t.clone() for t in a]
            rs = torch.tensor(3.0, dtype=torch.float64, device="cuda")
            pq = torch.tensor(4.0, dtype=torch.float64, device="cuda")
            old = torch.zeros((), dtype=torch.float64, device="cuda")
            if buf is not None:
                _poison(buf, old)
            ext.halo_cg_update_nd(x, r, b, outs, *_geom(st), rs, pq, old,
                                  part if buf is None else buf)
            got = [rs, old] + x + r
            if ref is None:
                ref = got
            assert old.item() == 3.0
            for g, e in zip(got, ref):
                assert torch.equal(g, e) and torch.isfinite(g).all()


# ------------------------------------------------------------------ solve

@pytest.mark.parametrize("periodic", SPD_PERIODIC)
@pytest.mark.parametrize("w", [1, 2])
def test_solve_table_on_the_gpu(grids, periodic, w):
    """The CPU suite's table with the same caps; both solutions have a
    true residual <= 2 * rtol * ||b|| and lambda_min(A) >= 1, so they
    differ by at most 4 * rtol * ||b||."""
    grid = grids[periodic]
    k = spd_weights(w)
    for dtype, rtol, cap in SOLVES:
        b = spd_rhs(w, dtype)
        cpu, _ = grid.make_stencil(b.shape, dtype, "cpu", k).make_cg().solve(
            b, rtol=rtol, maxiter=cap, check_every=1)
        st = grid.make_stencil(b.shape, dtype, "cuda", k)
        x, info = st.make_cg().solve(b.cuda(), rtol=rtol, maxiter=cap,
                                     check_every=1)
        assert info.converged is True and info.iterations <= cap
        true = true_residual(grid, k, x, b)
        print(periodic, w, dtype, info.iterations, true / rtol)
        assert true <= 2 * rtol, (periodic, w, dtype, true)
        bnorm = interior(b, w).double().norm().item()
        err = (x.cpu().double() - cpu.double()).norm().item()
        assert err <= 4 * rtol * bnorm, (periodic, w, dtype, err)
        assert not (x.cpu() - cpu)[..., :w, :].any(), "halo written"
        # no host read: exactly cap iterations
        x0, info0 = st.make_cg().solve(b.cuda(), rtol=rtol, maxiter=cap,
                                       check_every=0)
        assert info0.converged is None and info0.iterations == cap
        assert true_residual(grid, k, x0, b) <= 2 * rtol


def test_solve_is_reproducible(grids):
    torch.manual_seed(23)
    for periodic, dtype in itertools.product(SPD_PERIODIC,
                                             (torch.float32, torch.float64)):
        shape, w = (3, 41, 70), 2
        st = grids[periodic].make_stencil(shape, dtype, "cuda",
                                          spd_weights(w), nfields=2)
        b = [torch.randn(shape, dtype=dtype, device="cuda")
             for _ in range(2)]
        runs = []
        for _ in range(2):
            cg = st.make_cg()
            x, info = cg.solve(b, rtol=1e-5, maxiter=30)
            assert info.converged
            runs.append(list(x) + [cg.rs.clone()])
        for a, c in zip(*runs):
            assert torch.equal(a, c), (periodic, dtype)


# ------------------------------------------------------------- large sizes

def test_more_than_65535_planes(grids):
    """70000 planes of one interior cell: 70000 partials, which the finish
    kernel adds in 274 passes of 256, the last one ragged."""
    shape, w = (70000, 3, 3), 1
    k = make_weights("asym", w)
    for periodic in ((True, True), (True, False)):
        grid = grids[periodic]
        x = int_data(shape, torch.float32, 9)
        y = int_data(shape, torch.float32, 10)
        st = grid.make_stencil(shape, torch.float32, "cuda", k)
        assert st._partials_buf().numel() == 70000
        assert st.dot(x.cuda(), y.cuda()).item() == int_dot(
            interior(x, w), interior(y, w))
        (exp,) = oracle_apply(grid, k, [x])
        out, pap = st.apply_dot(x.cuda())
        assert torch.equal(interior(out.cpu(), w).double(), exp)
        assert pap.item() == int_dot(interior(x, w), exp)


def test_block_count_limit(grids):
    """2^24 planes of (3, 3) would be 2^24 blocks: every entry raises
    ValueError before anything is enqueued, by direct call."""
    n = 1 << 24
    ext = _ext()
    x = o = o2 = None
    try:
        x = torch.ones(n, 3, 3, device="cuda")
        o = torch.full((n, 3, 3), 7.0, device="cuda")
        o2 = torch.full((n, 3, 3), 7.0, device="cuda")
        part = torch.full((64,), 7.0, dtype=torch.float64, device="cuda")
        s = [torch.full((), 7.0, dtype=torch.float64, device="cuda")
             for _ in range(3)]
        big = grids[(True, True)].make_stencil((n, 3, 3), torch.float32,
                                               "cuda", [[0, 0, 0], [0, 2, 0],
                                                        [0, 0, 3]])
        ex = big.exchanger
        calls = (
            lambda: ext.halo_stencil_dot_nd(
                [x], [o], n, 3, 3, 1, [0, 1], [0, 1], [2.0, 3.0],
                ex._send_to, ex._recv_from, ex._local_mask, ex._sbuf,
                ex._rbuf, -1, part, s[0]),
            lambda: ext.halo_interior_dot_nd([x], [x], n, 3, 3, 1, part,
                                             s[0]),
            lambda: ext.halo_cg_update_nd([o], [o2], [x], [x], n, 3, 3, 1,
                                          s[0], s[1], s[2], part),
            lambda: ext.halo_cg_direction_nd([o], [x], n, 3, 3, 1, s[0],
                                             s[1]),
            lambda: big.apply_dot(x, out=o),
            lambda: big.dot(x, x),
        )
        for call in calls:
            with pytest.raises(ValueError, match="2\\^24"):
                call()
        torch.cuda.synchronize()
        assert bool((o == 7.0).all()) and bool((o2 == 7.0).all())
        assert bool((part == 7.0).all())
        assert all(t.item() == 7.0 for t in s)
    finally:
        del x, o, o2
        torch.cuda.empty_cache()


# ------------------------------------------------------ capture, validation

def test_graph_capture_and_no_allocation(grids):
    shape, w, nf = (3, 41, 70), 2, 2
    grid = grids[(True, True)]
    k = spd_weights(w)
    torch.manual_seed(9)
    for dtype in (torch.float32, torch.float64):
        st = grid.make_stencil(shape, dtype, "cuda", k, nfields=nf)
        cg = st.make_cg()
        b = [torch.randn(shape, dtype=dtype, device="cuda")
             for _ in range(nf)]
        x = [torch.zeros_like(t) for t in b]
        cg.start(b, x)
        cg.iterate(5)  # warm-up
        torch.cuda.synchronize()
        n0 = torch.cuda.memory_stats()["allocation.all.allocated"]
        cg.iterate(5)
        torch.cuda.synchronize()
        assert torch.cuda.memory_stats()["allocation.all.allocated"] == n0, \
            "iterate allocated after its warm-up"

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            cg.iterate(5)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):  # captures on a side stream
            cg.iterate(5)

        fresh = [torch.randn(shape, dtype=dtype, device="cuda")
                 for _ in range(nf)]
        eager = grid.make_stencil(shape, dtype, "cuda", k,
                                  nfields=nf).make_cg()
        ex_ = [torch.zeros_like(t) for t in fresh]
        eager.start(fresh, ex_)
        eager.iterate(5)
        for t in x:
            t.zero_()
        cg.start(fresh, x)  # the same x tensors the graph updates
        graph.replay()
        torch.cuda.synchronize()
        got = x + list(cg.residual) + list(cg.direction) + [cg.rs, cg.pq]
        want = (ex_ + list(eager.residual) + list(eager.direction)
                + [eager.rs, eager.pq])
        for a, c in zip(got, want):
            assert torch.equal(a, c), dtype
            assert a.abs().max() > 0


def test_native_entries_validate():
    """Every new pybind entry checks each argument itself and raises
    before anything is enqueued: one good call, then every bad argument,
    and the sentinel-filled outputs, partials and scalars are unchanged.
    halo_stencil_dot_nd shares halo_stencil_nd's checks of its first
    fifteen arguments (tests/test_gpu_halo_stencil.py); a sample of them
    and all of its own are here.  The block limit has its own test."""
    ext = _ext()
    dev = "cuda"

    def field(v, dtype=torch.float32):
        return torch.full((2, 9, 10), v, dtype=dtype, device=dev)

    def scalar(v):
        return torch.full((), v, dtype=torch.float64, device=dev)

    f, g = field(1.0), field(2.0)
    o, o2 = field(7.0), field(7.0)
    pair = torch.ones(2, 2, 9, 10, device=dev)
    part = torch.full((16,), 7.0, dtype=torch.float64, device=dev)
    res, rs, pq, old = scalar(7.0), scalar(3.0), scalar(4.0), scalar(7.0)
    buf = torch.zeros(4096, device=dev)
    wrap = [0, 0] + [-1] * 6
    fh = field(1.0, torch.bfloat16)
    oh = field(7.0, torch.bfloat16)
    fi = torch.ones(2, 9, 10, dtype=torch.int32, device=dev)

    bad_part = (part[:1], part.float(), part.cpu(),
                torch.zeros(32, dtype=torch.float64, device=dev)[::2])
    bad_scalar = (scalar(0.0).float(), scalar(0.0).cpu(),
                  torch.zeros(2, dtype=torch.float64, device=dev),
                  torch.zeros(1, 1, dtype=torch.float64, device=dev))
    bad_fields = ([], [f] * 9, [f.cpu()], [f.transpose(1, 2)], [f.double()],
                  [fi], [f, g], [torch.ones(2, 9, 11, device=dev)])
    bad_geom = (dict(width=0), dict(width=5), dict(width=4), dict(ny=10),
                dict(levels=3), dict(levels=0), dict(nx=9))

    def run(entry, names, ok, bads, outputs):
        def call(**kw):
            args = dict(zip(names, ok))
            args.update(kw)
            entry(*(args[n] for n in names))

        call()
        torch.cuda.synchronize()
        for t in (o, o2, part, res, old):
            t.fill_(7.0)
        rs.fill_(3.0)
        keep = [t.clone() for t in outputs]
        for bad in bads:
            with pytest.raises((RuntimeError, ValueError)):
                call(**bad)
        torch.cuda.synchronize()
        for t, kp in zip(outputs, keep):
            assert torch.equal(t, kp), "a refused call wrote something"
        assert torch.equal(f, field(1.0)) and torch.equal(g, field(2.0))
        assert torch.equal(pair, torch.ones_like(pair))

    # ---- halo_interior_dot_nd
    names = ("a", "b", "levels", "ny", "nx", "width", "partials", "result")
    ok = ([f], [g], 2, 9, 10, 2, part, res)
    bads = ([dict(a=v) for v in bad_fields]
            + [dict(b=v) for v in bad_fields]
            + [dict(a=[fh], b=[f]), dict(a=[fi], b=[fi])]
            + list(bad_geom)
            + [dict(partials=v) for v in bad_part]
            + [dict(result=v) for v in bad_scalar]
            + [dict(result=part[3:4])])
    run(ext.halo_interior_dot_nd, names, ok, bads, [part, res])
    # the 16-bit types are accepted here
    ext.halo_interior_dot_nd([fh], [fh], 2, 9, 10, 2, part, res)
    assert res.item() == 2 * 5 * 6
    part.fill_(7.0)
    res.fill_(7.0)

    # ---- halo_cg_update_nd
    names = ("x", "r", "p", "q", "levels", "ny", "nx", "width", "rs", "pq",
             "rs_old", "partials")
    ok = ([o], [o2], [f], [g], 2, 9, 10, 2, rs, pq, old, part)
    bads = ([dict([(n, v)]) for n in ("x", "r", "p", "q")
             for v in bad_fields]
            + [dict(x=[oh], r=[oh.clone()], p=[fh], q=[fh.clone()])]
            + list(bad_geom)
            + [dict(partials=v) for v in bad_part]
            + [dict([(n, v)]) for n in ("rs", "pq", "rs_old")
               for v in bad_scalar]
            # overlaps: written against read and written, scalars
            + [dict(x=[f]), dict(r=[g]), dict(r=[o]), dict(x=[o2]),
               dict(x=[pair[0]], p=[pair.view(-1)[90:270].view(2, 9, 10)]),
               dict(pq=rs), dict(rs_old=rs), dict(rs_old=pq),
               dict(rs=part[2:3]), dict(rs_old=part[0:1])])
    run(ext.halo_cg_update_nd, names, ok, bads, [o, o2, part, old, rs, pq])

    # ---- halo_cg_direction_nd
    names = ("p", "r", "levels", "ny", "nx", "width", "rs", "rs_old")
    ok = ([o], [f], 2, 9, 10, 2, rs, pq)
    bads = ([dict([(n, v)]) for n in ("p", "r") for v in bad_fields]
            + [dict(p=[oh], r=[fh])]
            + list(bad_geom)
            + [dict([(n, v)]) for n in ("rs", "rs_old") for v in bad_scalar]
            + [dict(p=[f]), dict(r=[o]),
               dict(p=[pair[0]], r=[pair.view(-1)[90:270].view(2, 9, 10)])])
    run(ext.halo_cg_direction_nd, names, ok, bads, [o, rs, pq])

    # ---- halo_stencil_dot_nd
    names = ("fields", "outs", "levels", "ny", "nx", "width", "tap_dy",
             "tap_dx", "tap_coef", "send_to", "recv_from", "local_mask",
             "sbuf", "rbuf", "comm_id", "partials", "result")
    ok = ([f], [o], 2, 9, 10, 2, [0, -2, 2], [0, 2, -1], [1.0, 2.0, 3.0],
          wrap, wrap, 0b11, buf, buf.clone(), -1, part, res)
    bads = ([dict(fields=[], outs=[]), dict(width=0), dict(width=4),
             dict(ny=10), dict(levels=3), dict(local_mask=256),
             dict(sbuf=buf[:8]), dict(fields=[f.cpu()]),
             dict(tap_dy=[0, 3, 2]), dict(tap_coef=[1.0]),
             dict(outs=[]), dict(outs=[o.double()]), dict(outs=[f]),
             dict(fields=[fi], outs=[fi.clone()]),
             dict(local_mask=0, comm_id=123456)]
            + [dict(partials=v) for v in bad_part]
            + [dict(result=v) for v in bad_scalar]
            + [dict(result=part[3:4])])
    run(ext.halo_stencil_dot_nd, names, ok, bads, [o, part, res])
