"""GPU suite for parallel/chebyshev.StencilChebyshev: the native executor
(the CHEB epilogue of csrc/stencil.hip behind the bridge.cpp entry
halo_cheb_step_nd) at world 1.

Oracles, data and the SPD system are those of
tests/test_stencil_chebyshev.py.  The two exact steps are compared with
exact arithmetic for both executors, hence bitwise with each other; the
fused multiply-adds of the kernel change roundings only, so everything
else is held to the same bounds as on the CPU.
"""

import itertools
import math

import pytest
import torch

import mpi4jax_amd as m
from mpi4jax_amd.parallel.grid import CartesianGrid
from test_gpu_halo_exchanger import OPEN, _valid
from test_halo_adjoint import int_data
from test_halo_stencil import as_tuple, interior, make_weights
from test_stencil_cg import SPD_PERIODIC, spd_weights
from test_stencil_chebyshev import check_exact_steps, check_solve_table

pytestmark = pytest.mark.gpu

ALL = OPEN + [(False, False)]
F32_F64 = (torch.float32, torch.float64)
# n == 3 * width and 3 * width + 1 at width 4; batch dims; several 32 x 64
# tiles with ragged edges; and the one shape with a tile on the stencil
# kernel's fast fill at every width, so CHEB runs after both fills
SHAPES = [(12, 12), (13, 12), (2, 9, 10), (3, 41, 70), (2, 76, 140)]
NFS = (1, 3, 8)


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
        v = t.view(torch.int32 if t.element_size() == 4 else torch.int64)
        v.fill_(-1)  # all bits set: a NaN


def _native_args(st):
    ex = st.exchanger
    return (ex.levels, ex.ny, ex.nx, st.width, st._tap_dy, st._tap_dx,
            st._tap_coef, ex._send_to, ex._recv_from, ex._local_mask,
            ex._sbuf, ex._rbuf, -1)


# ------------------------------------------------- two exact steps, bitwise

@pytest.mark.parametrize("periodic", ALL)
@pytest.mark.parametrize("w", [1, 2, 3, 4])
def test_two_steps_native_python_and_exact_arithmetic_agree(
        grids, periodic, w, monkeypatch):
    """Every width with every ``nf`` in (1, 3, 8) on the three small
    shapes and both executors; on the two large shapes the native executor
    with ``nf`` and dtype alternating over the cases (the Python executor
    does nothing there that it does not do on the small ones)."""
    grid = grids[periodic]
    ran = 0
    for si, shape in enumerate(SHAPES):
        if not _valid(shape, w):
            continue
        small = shape[-1] < 64
        for ni, nf in enumerate(NFS):
            if not small and ni != (si + w) % 3:
                continue
            for di, dtype in enumerate(F32_F64):
                if not small and di != (w + int(periodic[0])) % 2:
                    continue
                for env in (None, "1") if small else (None,):
                    if env:
                        monkeypatch.setenv("MPI4JAX_AMD_HALO_PY", env)
                    else:
                        monkeypatch.delenv("MPI4JAX_AMD_HALO_PY",
                                           raising=False)
                    check_exact_steps(grid, shape, w, nf, dtype,
                                      device="cuda")
                    ran += 1
                monkeypatch.delenv("MPI4JAX_AMD_HALO_PY", raising=False)
    assert ran >= (3 if w < 4 else 2) * 3 * 2 * 2 + 2


# ------------------------------------------------------------ staged path

@pytest.mark.parametrize("periodic", OPEN)
def test_staged_path_equals_direct_path_bitwise(grids, periodic):
    """``_force_remote`` sends the strips of ``d`` to self through the
    RCCL group and the kernel reads the receive slots; the arithmetic is
    the same.  The direct path creates no communicator."""
    grid = grids[periodic]
    torch.manual_seed(5)
    for (shape, w), dtype in itertools.product(
            [((2, 9, 10), 2), ((3, 41, 70), 1), ((3, 41, 70), 4),
             ((2, 76, 140), 3)], F32_F64):
        if w <= 2:
            k = spd_weights(w)
        else:  # symmetric and diagonally dominant
            k = 0.01 * torch.randn(2 * w + 1, 2 * w + 1,
                                   dtype=torch.float64)
            k = k + k.flip(0, 1)
            k[w, w] = 1.0
        b = [torch.randn(shape, dtype=dtype, device="cuda")
             for _ in range(2)]
        res = {}
        for name in ("direct", "staged"):
            before = _ext().comm_count()
            st = grid.make_stencil(shape, dtype, "cuda", k, nfields=2,
                                   _force_remote=name == "staged")
            lo, hi = st.gershgorin_bounds()
            assert lo > 0
            ch = st.make_chebyshev(lo, hi)
            x = [torch.zeros_like(t) for t in b]
            ch.start(b, x)
            ch.iterate(5)
            res[name] = x + list(ch.residual) + list(ch.direction)
            if name == "direct":
                torch.cuda.synchronize()
                assert _ext().comm_count() == before, \
                    "the direct path created a communicator"
            else:
                assert not st.exchanger.local_directions
        for a, c in zip(res["direct"], res["staged"]):
            assert torch.equal(a, c), (shape, w, dtype)
            assert torch.isfinite(a).all() and a.abs().max() > 0


# ------------------------------------------------------------------ solve

@pytest.mark.parametrize("periodic", SPD_PERIODIC)
@pytest.mark.parametrize("w", [1, 2])
def test_solve_table_on_the_gpu(grids, periodic, w):
    """The CPU suite's table with the same bounds and the same counts."""
    check_solve_table(grids[periodic], w, device="cuda")


def test_solve_is_reproducible(grids):
    torch.manual_seed(23)
    for periodic, dtype in itertools.product(SPD_PERIODIC, F32_F64):
        shape, w = (3, 41, 70), 2
        st = grids[periodic].make_stencil(shape, dtype, "cuda",
                                          spd_weights(w), nfields=2)
        b = [torch.randn(shape, dtype=dtype, device="cuda")
             for _ in range(2)]
        runs = []
        for _ in range(2):
            ch = st.make_chebyshev(1, 11 / 3)
            x, info = ch.solve(b, rtol=1e-5)
            assert info.converged
            runs.append(list(x) + list(ch.residual) + [info.residual_norm])
        for a, c in zip(*runs):
            assert (torch.equal(a, c) if isinstance(a, torch.Tensor)
                    else a == c), (periodic, dtype)


# --------------------------------------------------------------- poisoning

def test_poisoned_outputs_and_unread_halos(grids):
    """What the kernel must not read holds the NaN pattern and changes
    nothing: the interior of ``d_out`` before every step, the halo of
    ``b``, and the halo of ``x`` along periodic edges (the stencil is a
    star, so no halo corner is read either).  The reference run has zeros
    there."""
    for periodic, (shape, w), dtype in itertools.product(
            ALL, [((2, 9, 10), 2), ((3, 41, 70), 1), ((2, 76, 140), 4)],
            F32_F64):
        grid = grids[periodic]
        k = make_weights("star", w, seed=2)
        k[w, w] = 60.0  # diagonally dominant: the iterates stay small
        st = grid.make_stencil(shape, dtype, "cuda", k, nfields=2)
        lo, hi = st.gershgorin_bounds()
        assert lo > 0
        runs = []
        for poisoned in (False, True):
            b = [int_data(shape, dtype, 40 + i, "cuda") for i in range(2)]
            x = [torch.zeros(shape, dtype=dtype, device="cuda")
                 for _ in range(2)]
            for t in b:
                keep = interior(t, w).clone()
                if poisoned:
                    _poison(t)
                else:
                    t.zero_()
                interior(t, w).copy_(keep)
            if poisoned:
                for t in x:
                    if periodic[0]:
                        _poison(t[..., :w, :], t[..., -w:, :])
                    if periodic[1]:
                        _poison(t[..., :, :w], t[..., :, -w:])
                    interior(t, w).zero_()
                    assert torch.isnan(t).any() == any(periodic)
            ch = st.make_chebyshev(lo, hi)
            ch.start(b, x)
            for _ in range(4):
                if poisoned:
                    for t in ch._d[1 - ch._cur]:
                        _poison(interior(t, w))
                ch.iterate(1)
            runs.append([interior(t, w) for t in x]
                        + list(ch.residual) + list(ch.direction))
        for a, c in zip(*runs):
            assert torch.isfinite(c).all(), (periodic, shape, w, dtype)
            assert torch.equal(a, c), (periodic, shape, w, dtype)
            assert a.abs().max() > 0


# ------------------------------------------------------ capture, validation

def test_graph_capture_and_no_allocation(grids):
    shape, w, nf = (3, 41, 70), 2, 2
    grid = grids[(True, True)]
    k = spd_weights(w)
    torch.manual_seed(9)
    for dtype in F32_F64:
        st = grid.make_stencil(shape, dtype, "cuda", k, nfields=nf)
        ch = st.make_chebyshev(1, 11 / 3)
        b = [torch.randn(shape, dtype=dtype, device="cuda")
             for _ in range(nf)]
        x = [torch.zeros_like(t) for t in b]
        ch.start(b, x)
        ch.iterate(6)  # warm-up
        torch.cuda.synchronize()
        n0 = torch.cuda.memory_stats()["allocation.all.allocated"]
        bytes0 = torch.cuda.memory_allocated()
        ch.iterate(6)
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == bytes0
        assert torch.cuda.memory_stats()["allocation.all.allocated"] == n0, \
            "iterate allocated after its warm-up"

        # capture iterations 0..5: the graph holds their coefficients
        for t in x:
            t.zero_()
        ch.start(b, x)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ch.iterate(6)
        torch.cuda.current_stream().wait_stream(side)
        for t in x:
            t.zero_()
        ch.start(b, x)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):  # captures on a side stream
            ch.iterate(6)
        assert ch.iteration == 6

        eager = grid.make_stencil(shape, dtype, "cuda", k,
                                  nfields=nf).make_chebyshev(1, 11 / 3)
        ex_ = [torch.zeros_like(t) for t in b]
        eager.start(b, ex_)
        eager.iterate(6)
        for t in x:
            t.zero_()
        ch.start(b, x)  # the same x tensors the graph updates
        graph.replay()
        torch.cuda.synchronize()
        got = x + list(ch.residual) + list(ch._d[0])
        want = ex_ + list(eager.residual) + list(eager.direction)
        for a, c in zip(got, want):
            assert torch.equal(a, c), dtype
            assert a.abs().max() > 0


def test_native_entry_validates():
    """halo_cheb_step_nd checks its arguments itself and raises before
    anything is enqueued: one good call, then the bad ones, and the
    sentinel-filled buffers are unchanged.  It shares halo_stencil_nd's
    checks of the taps, the geometry and the staging buffers
    (tests/test_gpu_halo_stencil.py); a sample of them and all of its own
    are here."""
    ext = _ext()
    dev = "cuda"

    def field(v, dtype=torch.float32):
        return torch.full((2, 9, 10), v, dtype=dtype, device=dev)

    d, o, x, r = field(1.0), field(7.0), field(7.0), field(7.0)
    pair = torch.full((2, 2, 9, 10), 7.0, device=dev)
    shifted = pair.view(-1)[90:270].view(2, 9, 10)
    buf = torch.zeros(4096, device=dev)
    wrap = [0, 0] + [-1] * 6
    names = ("d_in", "d_out", "x", "r", "levels", "ny", "nx", "width",
             "tap_dy", "tap_dx", "tap_coef", "send_to", "recv_from",
             "local_mask", "sbuf", "rbuf", "comm_id", "c1", "c2")
    ok = ([d], [o], [x], [r], 2, 9, 10, 2, [0, -2, 2], [0, 2, -1],
          [1.0, 2.0, 3.0], wrap, wrap, 0b11, buf, buf.clone(), -1, 0.5,
          0.25)

    def call(**kw):
        args = dict(zip(names, ok))
        args.update(kw)
        ext.halo_cheb_step_nd(*(args[n] for n in names))

    call()
    torch.cuda.synchronize()
    assert torch.equal(interior(x, 2), torch.full((2, 5, 6), 8.0,
                                                  device=dev))
    for t in (o, x, r):
        t.fill_(7.0)
    h = [field(1.0, torch.bfloat16) for _ in range(4)]
    hh = [field(1.0, torch.float16) for _ in range(4)]
    fi = [torch.ones(2, 9, 10, dtype=torch.int32, device=dev)
          for _ in range(4)]
    bad_fields = ([], [d, d.clone()], [d.cpu()], [d.transpose(1, 2)],
                  [d.double()], [torch.ones(2, 9, 11, device=dev)])
    bads = (
        # 16-bit and integer dtypes
        [dict(d_in=[t[0]], d_out=[t[1]], x=[t[2]], r=[t[3]])
         for t in (h, hh, fi)]
        + [dict([(n, v)]) for n in ("d_in", "d_out", "x", "r")
           for v in bad_fields]
        # aliasing: every pair of the four lists, and a partial overlap
        + [dict(d_out=[d]), dict(x=[d]), dict(r=[d]), dict(x=[o]),
           dict(r=[o]), dict(r=[x]), dict(x=[r]),
           dict(x=[pair[0]], r=[shifted]),
           dict(d_out=[pair[0]], x=[shifted]),
           dict(d_in=[pair[0]], r=[shifted]),
           dict(x=[buf[:180].view(2, 9, 10)])]
        + [dict(c1=v) for v in (math.inf, -math.inf, math.nan)]
        + [dict(c2=v) for v in (math.inf, -math.inf, math.nan)]
        + [dict(width=0), dict(width=4), dict(width=5), dict(ny=10),
           dict(levels=3), dict(local_mask=256), dict(sbuf=buf[:8]),
           dict(tap_dy=[0, 3, 2]), dict(tap_coef=[1.0]),
           dict(local_mask=0, comm_id=123456)])
    for bad in bads:
        with pytest.raises((RuntimeError, ValueError, TypeError)):
            call(**bad)
    torch.cuda.synchronize()
    for t in (o, x, r):
        assert torch.equal(t, field(7.0)), "a refused call wrote something"
    assert torch.equal(d, field(1.0))
    assert torch.equal(pair, torch.full_like(pair, 7.0))
    assert not buf.any()


def test_block_count_limit(grids):
    """2^24 planes of (3, 3) would be 2^24 blocks: ValueError before
    anything is enqueued."""
    n = 1 << 24
    t = None
    try:
        t = [torch.full((n, 3, 3), 7.0, device="cuda") for _ in range(4)]
        big = grids[(True, True)].make_stencil(
            (n, 3, 3), torch.float32, "cuda", [[0, 0, 0], [0, 2, 0],
                                                [0, 0, 3]])
        ex = big.exchanger
        with pytest.raises(ValueError, match="2\\^24"):
            _ext().halo_cheb_step_nd(
                [t[0]], [t[1]], [t[2]], [t[3]], n, 3, 3, 1, [0, 1], [0, 1],
                [2.0, 3.0], ex._send_to, ex._recv_from, ex._local_mask,
                ex._sbuf, ex._rbuf, -1, 0.5, 0.5)
        ch = big.make_chebyshev(1, 5)
        ch._x = [t[2]]  # as after start, which would refuse as well
        with pytest.raises(ValueError, match="2\\^24"):
            ch.step(0.5, 0.5)
        torch.cuda.synchronize()
        assert all(bool((v == 7.0).all()) for v in t)
    finally:
        del t
        torch.cuda.empty_cache()
