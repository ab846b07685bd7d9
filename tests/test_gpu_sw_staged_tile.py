"""GPU tests: the LDS-staged fast tiles of the single-launch world-1
shallow-water step (stage 30/31, kernel ``sw_step1t``).

A fast tile loads the 18 x 66 window of h, u and v it needs into LDS once
and computes its 16 x 32 fill pairs from there; perimeter tiles keep the
global-load form.  Neither comparison path below runs that code: the
three-launch form (``MPI4JAX_AMD_SW_RING3=1``, stage 34) and the
two-kernel path (``MPI4JAX_AMD_SW_NOFUSE=1``, stage 19) load every pair's
stencil from global memory.  Same formulas, different FMA-contraction
sites, so the tolerances are the project's for exactly this comparison
(step 1: atol 2e-6 / rtol 1e-6; step 9: atol 5e-5 / rtol 1e-4), over the
FULL local arrays, halo ring included.

Which tiles are fast (``s1_tiles`` in ``csrc/shallow_water.hip``).  The
local grid is (ny+2) x (nx+2); tile (tr, tc) owns rows 14*tr .. 14*tr+13
and columns 60*tc .. 60*tc+59, and is fast iff its fill rows
14*tr-1 .. 14*tr+14 lie in [jmin, jmax] and its fill pairs, first columns
60*tc-2 .. 60*tc+60, lie in [imin, ihi] with ihi = min(imax-2, nx+2-4).
``SW_FAST_BOUNDS`` with closed edges gives jmin = 2, jmax = ny-1, imin = 2,
imax = nx, so ihi = nx-2:

* rows: 14*tr-1 >= 2 and 14*tr+14 <= ny-1, i.e. 1 <= tr and
  14*tr + 15 <= ny;
* columns: 60*tc-2 >= 2 and 60*tc+60 <= nx-2, i.e. 1 <= tc and
  60*tc + 62 <= nx.

With ``periodic_x`` the x halos are open and there is no east wall:
imin = 1, imax = nx+1, ihi = min(nx-1, nx-2) = nx-2 still (the 4-wide row
load must end inside the row), and 60*tc-2 >= 1 still needs tc >= 1: the
same fast columns.  y is never periodic.  So:

* nx in {182, 183, 184, 185}, ny = 43: tr, tc in {1, 2}, the smallest
  domain with a 2 x 2 block of fast tiles (aprons shared fast-fast both
  ways and fast-perimeter on all four sides); the row pitch nx+2 takes all
  four residues mod 4, every misalignment of the staging loads; at
  nx = 182 the last staged column, 60*2+62 = 182, is one short of the
  row's last, the closest the bounds allow;
* (122, 29): exactly one fast tile, surrounded by perimeter tiles;
* (250, 100): a fast rectangle of tile columns 1..3 and tile rows 1..6.
"""

import functools

import pytest
import torch

import mpi4jax_amd as m

pytestmark = pytest.mark.gpu

FIELDS = ("h", "u", "v", "dh", "du", "dv")
ENVS = ("MPI4JAX_AMD_SW_RING3", "MPI4JAX_AMD_SW_NOFUSE",
        "MPI4JAX_AMD_SW_FUSE512", "MPI4JAX_AMD_SW_GRAPH")
SHAPES = [(182, 43), (183, 43), (184, 43), (185, 43), (122, 29), (250, 100)]
MODES = {"single": ({}, 30),
         "ring3": ({"MPI4JAX_AMD_SW_RING3": "1"}, 34),
         "nofuse": ({"MPI4JAX_AMD_SW_NOFUSE": "1"}, 19),
         "fuse512": ({"MPI4JAX_AMD_SW_FUSE512": "1"}, 31)}


@pytest.fixture(scope="module", autouse=True)
def _init():
    m.init()
    yield
    torch.cuda.synchronize()


def _snap(st):
    # the model double-buffers in place: snapshot by value
    return {k: getattr(st, k).clone() for k in FIELDS}


@functools.lru_cache(maxsize=None)
def _trajectory(nx, ny, periodic, mode):
    """(state after the Euler step, state after 8 more steps) of one path;
    computed once per (shape, path) and shared between the tests."""
    from mpi4jax_amd.models import ShallowWater

    env, stage = MODES[mode]
    with pytest.MonkeyPatch.context() as mp:
        for k in ENVS:
            mp.delenv(k, raising=False)
        for k, v in env.items():
            mp.setenv(k, v)
        sw = ShallowWater(nx=nx, ny=ny, device="cuda", fused=True,
                          periodic_x=periodic, comm=m.get_world().Clone())
        assert sw._stage_plan()[1] == stage
        st = sw.step(sw.initial_conditions(), first_step=True)
        torch.cuda.synchronize()
        first = _snap(st)
        for _ in range(8):
            st = sw.step(st)
        torch.cuda.synchronize()
        return first, _snap(st)


def _assert_close(nx, ny, periodic, other):
    new = _trajectory(nx, ny, periodic, "single")
    old = _trajectory(nx, ny, periodic, other)
    for name in FIELDS:
        a1, b1 = old[0][name], new[0][name]
        d1 = (a1 - b1).abs().max().item()
        a9, b9 = old[1][name], new[1][name]
        d9 = (a9 - b9).abs().max().item()
        print(f"{other} ({nx},{ny}) periodic={periodic} {name}: "
              f"step1 max|d|={d1:.3e} step9 max|d|={d9:.3e}")
        assert torch.isfinite(b9).all(), (name, "non-finite")
        assert a1.shape == (ny + 2, nx + 2)
        assert torch.allclose(a1, b1, atol=2e-6, rtol=1e-6), (
            "step1", name, d1)
        assert torch.allclose(a9, b9, atol=5e-5, rtol=1e-4), (
            "step9", name, d9)


@pytest.mark.parametrize("periodic", [True, False])
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_staged_tiles_match_three_launch(nx, ny, periodic):
    _assert_close(nx, ny, periodic, "ring3")


@pytest.mark.parametrize("periodic", [True, False])
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_staged_tiles_match_two_kernel_path(nx, ny, periodic):
    _assert_close(nx, ny, periodic, "nofuse")


def test_staged_512thread_variant_is_bitwise():
    """Stage 31 runs the same per-task code over the same window."""
    a = _trajectory(185, 43, False, "single")
    b = _trajectory(185, 43, False, "fuse512")
    for i in (0, 1):
        for name in FIELDS:
            d = (a[i][name] - b[i][name]).abs().max().item()
            assert torch.equal(a[i][name], b[i][name]), (i, name, d)


def test_staged_graph_replay_matches_plain_steps(monkeypatch):
    """make_stepper(steps_per_call=4) equals four plain step calls bitwise
    (after its two warm-up steps), replayed twice."""
    from mpi4jax_amd.models import ShallowWater

    for k in ENVS:
        monkeypatch.delenv(k, raising=False)
    out = {}
    for graphed in (False, True):
        sw = ShallowWater(nx=185, ny=43, device="cuda", fused=True,
                          comm=m.get_world().Clone())
        assert sw._stage_plan()[1] == 30
        st = sw.step(sw.initial_conditions(), first_step=True)
        if graphed:
            advance, st = sw.make_stepper(st, steps_per_call=4)
            advance()
            st = advance()
        else:
            for _ in range(2 + 4 + 4):
                st = sw.step(st)
        torch.cuda.synchronize()
        out[graphed] = _snap(st)
    for name in FIELDS:
        assert torch.equal(out[False][name], out[True][name]), name
