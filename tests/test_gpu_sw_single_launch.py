"""GPU tests: the single-launch world-1 shallow-water step (stage 30/31,
kernel ``sw_step1t``) against the paths it replaces.

The single launch must write everything the three-launch form (fast
kernel + ringA + ringB, ``MPI4JAX_AMD_SW_RING3=1``) writes: same
formulas, different FMA-contraction sites, so the comparison uses the
tolerances of ``test_stage30_matches_two_kernel_path`` (step 1: atol
2e-6 / rtol 1e-6; step 9: atol 5e-5 / rtol 1e-4) over the FULL local
arrays, halo ring included.  Shapes are chosen against the 14-row x
60-column tile partition of the (ny+2) x (nx+2) local grid: all-perimeter
domains, ny < 8, exactly one tile, a one-column sliver tile, a few fast
tiles surrounded by perimeter tiles, and tile edges on interior
rows/columns.
"""

import functools

import pytest
import torch

import mpi4jax_amd as m

pytestmark = pytest.mark.gpu

FIELDS = ("h", "u", "v", "dh", "du", "dv")
ENVS = ("MPI4JAX_AMD_SW_RING3", "MPI4JAX_AMD_SW_NOFUSE",
        "MPI4JAX_AMD_SW_FUSE512")
SHAPES = [(8, 32), (64, 5), (58, 12), (59, 13), (120, 60), (130, 66),
          (53, 37), (1040, 24), (185, 44)]
MODES = {"single": ({}, 30), "ring3": ({"MPI4JAX_AMD_SW_RING3": "1"}, 34),
         "nofuse": ({"MPI4JAX_AMD_SW_NOFUSE": "1"}, 19)}


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
def test_single_launch_matches_three_launch(nx, ny, periodic):
    _assert_close(nx, ny, periodic, "ring3")


@pytest.mark.parametrize("periodic", [True, False])
@pytest.mark.parametrize("nx,ny", [(120, 60), (53, 37)])
def test_single_launch_matches_two_kernel_path(nx, ny, periodic):
    _assert_close(nx, ny, periodic, "nofuse")


@pytest.mark.parametrize("periodic", [True, False])
def test_single_launch_ignores_fe_fn_scratch(periodic, monkeypatch):
    """The u'/v' strip staging is gone: NaN-poisoned fe/fn scratch must
    not reach any output, from the very first step on."""
    from mpi4jax_amd.models import ShallowWater
    from mpi4jax_amd.models.shallow_water import ModelState

    for k in ENVS:
        monkeypatch.delenv(k, raising=False)
    nx, ny = 120, 60
    sw = ShallowWater(nx=nx, ny=ny, device="cuda", fused=True,
                      periodic_x=periodic, comm=m.get_world().Clone())
    assert sw._stage_plan()[1] == 30
    sw._init_fused_buffers(sw.initial_conditions())
    fb = sw._fb
    fb["fe"].fill_(float("nan"))
    fb["fn"].fill_(float("nan"))
    st = ModelState(fb["h"], fb["u"], fb["v"], fb["do_h"], fb["do_u"],
                    fb["do_v"])
    st = sw.step(st, first_step=True)
    assert sw._fb is fb  # the poisoned buffers are the ones stepped
    for _ in range(8):
        st = sw.step(st)
    torch.cuda.synchronize()
    assert torch.isnan(fb["fe"]).all() and torch.isnan(fb["fn"]).all()
    clean = _trajectory(nx, ny, periodic, "single")[1]
    for name in FIELDS:
        got = getattr(st, name)
        assert torch.isfinite(got).all(), name
        assert torch.equal(got, clean[name]), name


def test_single_launch_graph_replay_matches_plain_steps(monkeypatch):
    """make_stepper(steps_per_call=4) on the single-launch path equals
    four plain step calls bitwise (after its two warm-up steps)."""
    from mpi4jax_amd.models import ShallowWater

    for k in ENVS + ("MPI4JAX_AMD_SW_GRAPH",):
        monkeypatch.delenv(k, raising=False)
    out = {}
    for graphed in (False, True):
        sw = ShallowWater(nx=120, ny=60, device="cuda", fused=True,
                          comm=m.get_world().Clone())
        assert sw._stage_plan()[1] == 30
        st = sw.step(sw.initial_conditions(), first_step=True)
        if graphed:
            advance, st = sw.make_stepper(st, steps_per_call=4)
            st = advance()
        else:
            for _ in range(2 + 4):
                st = sw.step(st)
        torch.cuda.synchronize()
        out[graphed] = _snap(st)
    for name in FIELDS:
        assert torch.equal(out[False][name], out[True][name]), name


def test_stage_dispatch_is_explicit():
    """The native stage table equals the Python enum, and a launch the
    table cannot serve raises without launching anything: an id that is
    no stage, and a float32-only stage handed float64 buffers."""
    from mpi4jax_amd._backend import rccl
    from mpi4jax_amd.models.shallow_water import SwStage

    ext = rccl.ext()
    assert ext.sw_stage_ids() == {s.name: int(s) for s in SwStage}

    def call(stage, dtype):
        bufs = [torch.full((10, 34), 7.0, dtype=dtype, device="cuda")
                for _ in range(16)]
        with pytest.raises(RuntimeError):
            ext.sw_stage(stage, bufs, 5e3, 5e3, 10.0, 1.0, 2e-4, 1e-7, 1.0,
                         0.0, [0, 0, 1, 1, 0, 1, 1])
        torch.cuda.synchronize()
        assert all(bool((b == 7.0).all()) for b in bufs)

    call(9, torch.float32)
    call(30, torch.float64)
