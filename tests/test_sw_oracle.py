"""CPU tests of the shallow-water reference (tests/sw_oracle.py): it equals
the model's eager float64 step bitwise, its magnitude companion dominates
it, a float32 evaluation of it stays inside the bounds the GPU tests use
(so the bounds are satisfiable by a correct float32 implementation), and
the decomposition helpers tile and exchange exactly."""

import pytest
import torch

from mpi4jax_amd.models import ShallowWater
from mpi4jax_amd.models import shallow_water as sw_mod
import sw_oracle as o

F32, F64 = torch.float32, torch.float64


@pytest.mark.parametrize("periodic_x", [True, False])
@pytest.mark.parametrize("first_step", [True, False])
def test_oracle_equals_eager_step_bitwise(periodic_x, first_step):
    """Full arrays, rough state, random old tendencies, dx != dy."""
    ny, nx = 11, 17
    ab = ((1.0, 0.0) if first_step else
          (sw_mod.ADAMS_BASHFORTH_A, sw_mod.ADAMS_BASHFORTH_B))
    p = o.Params(**o.BASE, ab_a=ab[0], ab_b=ab[1], periodic_x=periodic_x)
    state = o.rough_state(ny, nx, periodic_x, seed=3)
    model = ShallowWater(nx=nx, ny=ny, dx=p.dx, dy=p.dy, device="cpu",
                         dtype=F64, periodic_x=periodic_x,
                         lateral_viscosity=p.nu, fused=False)
    model.dt = p.dt
    model.coriolis = o.coriolis(p, ny + 2, F64).expand(ny + 2, nx + 2)
    got = model.step(sw_mod.ModelState(*[x.clone() for x in state]),
                     first_step=first_step)
    ref = o.step(*state, p)
    for name, g in zip(("h1", "u2", "v2", "dnh", "dnu", "dnv"), got):
        assert torch.equal(g, ref[name]), name
    # the update changed every field by far more than rounding, and the
    # friction changed u, v again: no stage of the comparison is vacuous
    assert (ref["h1"] - state[0]).abs().mean() > 1e-2
    assert (ref["u2"] - ref["u1"]).abs().mean() > 1e-2


@pytest.mark.parametrize("cfg", o.CONFIGS, ids=str)
def test_magnitude_dominates(cfg):
    _, _, ref = o.case(*cfg, *o.SHAPES[1], o.AB[1], F32)
    for name in o._NAMES:
        assert (ref["mag_" + name] >= ref[name].abs()).all(), name


def _standin_ratios(cfg, shape, ab):
    """err / (u * mag) of a float32 torch evaluation of the reference, per
    stage family and output, against the float64 reference."""
    p, state, ref = o.case(*cfg, *shape, ab, F32)
    s32 = [x.to(F32) for x in state]
    r32 = {k: v.to(F32) for k, v in ref.items() if not k.startswith("mag_")}
    out = {}

    def put(family, names, arrays):
        for n, a in zip(names, arrays):
            out[family, n] = o.ratio(a, ref[n], ref["mag_" + n], F32)

    pre32 = o.pre(*s32[:3], p)
    put("pre", ("fe", "fn", "q", "ke"), pre32)
    upd = ("dnh", "dnu", "dnv", "h1", "u1", "v1")
    put("update2", upd,
        o.update(*[r32[k] for k in ("fe", "fn", "q", "ke")], *s32, p))
    merged = o.update(*pre32, *s32, p)
    put("merged", upd, merged)
    put("friction", ("u2", "v2"), o.friction(r32["u1"], r32["v1"], p))
    put("whole", ("u2", "v2"), o.friction(merged[4], merged[5], p))
    return out


_COUNTS = {"pre": o.N_PRE, "update2": o.N_UPDATE2, "merged": o.N_MERGED,
           "friction": o.N_FRICTION, "whole": o.N_WHOLE}


@pytest.mark.parametrize("cfg", o.CONFIGS, ids=str)
def test_float32_standin_inside_the_gpu_bounds(cfg):
    """The same reference evaluated in float32 (a stand-in for a correct
    kernel, division form) on exactly the GPU tests' inputs."""
    worst = {}
    for shape in o.SHAPES:
        for ab in o.AB:
            for key, r in _standin_ratios(cfg, shape, ab).items():
                worst[key] = max(worst.get(key, 0.0), r)
    for (family, name), r in sorted(worst.items()):
        k = o.bound_k(_COUNTS[family][name], F32)
        print(f"STANDIN {family} {name} ratio={r:.2f} K={k}")
    for (family, name), r in worst.items():
        assert r <= o.bound_k(_COUNTS[family][name], F32), (family, name, r)


def test_bounds_are_tight_enough_to_bite():
    """No K above 64 (a 1%-of-mag term error is a ratio near 1.7e5), and a
    wrong term is far outside: a Coriolis row offset of one (cor_dj), as
    a kernel mixing up corj and corjm would make, misses the dnu bound by
    more than 100x."""
    for family, table in _COUNTS.items():
        for n in table.values():
            assert o.bound_k(n, F32) <= 64
            if family != "whole":  # the fused step has no float64 kernel
                assert o.bound_k(n, F64) <= 64
    p, state, ref = o.case(1, 1, True, *o.SHAPES[1], o.AB[1], F32)
    fe, fn, q, ke = (ref[k] for k in ("fe", "fn", "q", "ke"))
    q_bad = o.pre(*state[:3], p._replace(cor0=p.cor0 + p.cor_dj))[2]
    bad = o.update(fe, fn, q_bad, ke, *state, p)
    r = o.ratio(bad[1], ref["dnu"], ref["mag_dnu"], F32)
    assert r > 100 * o.bound_k(o.N_MERGED["dnu"], F32), r


@pytest.mark.parametrize("cfg", o.CONFIGS, ids=str)
def test_tiles_tile_the_global_array(cfg):
    P, Q, periodic = cfg
    nyl, nxl = o.SHAPES[1]
    g = torch.arange((P * nyl + 2) * (Q * nxl + 2), dtype=F64).reshape(
        P * nyl + 2, Q * nxl + 2)
    tiles = o.cut(g, P, Q)
    assert len(tiles) == P * Q
    back = torch.full_like(g, -1.0)
    for (py, px), t in tiles.items():
        assert t.shape == (nyl + 2, nxl + 2)
        # interiors are disjoint and cover the global interior exactly
        sl = (slice(1 + py * nyl, 1 + (py + 1) * nyl),
              slice(1 + px * nxl, 1 + (px + 1) * nxl))
        assert (back[sl] == -1.0).all()
        back[sl] = t[1:-1, 1:-1]
        # the halo ring is the neighbours' (or the global halo's) data
        assert torch.equal(t, g[py * nyl:py * nyl + nyl + 2,
                                px * nxl:px * nxl + nxl + 2])
    assert torch.equal(back[1:-1, 1:-1], g[1:-1, 1:-1])


@pytest.mark.parametrize("cfg", o.CONFIGS, ids=str)
def test_exchange_reproduces_the_global_slices(cfg):
    P, Q, periodic = cfg
    nyl, nxl = o.SHAPES[0]
    g = o.rough_state(P * nyl, Q * nxl, periodic, seed=11)[0]
    want = o.cut(g, P, Q)
    tiles = o.cut(g, P, Q)
    nopen = 0
    for (py, px), t in tiles.items():
        s, n, w, e = o.tile_flags(P, Q, py, px, periodic)[:4]
        stale = torch.zeros_like(t, dtype=torch.bool)
        if s:
            stale[0, 1:-1] = True
        if n:
            stale[-1, 1:-1] = True
        if w:
            stale[:, 0] = True
        if e:
            stale[:, -1] = True
        t[stale] = float("nan")
        nopen += int(stale.sum())
    o.exchange(tiles, P, Q, periodic)
    for k in tiles:
        assert torch.equal(tiles[k], want[k]), k
    assert nopen > 0 or (P, Q, periodic) == (1, 1, False)


def test_flags_match_the_model():
    """tile_flags is ShallowWater._fused_flags for the world-1 model, and
    the x_wrap override is its _force_remote_exchange."""
    for periodic in (True, False):
        model = ShallowWater(nx=8, ny=6, device="cpu", periodic_x=periodic)
        assert o.tile_flags(1, 1, 0, 0, periodic) == model._fused_flags()
    forced = ShallowWater(nx=8, ny=6, device="cpu",
                          _force_remote_exchange=True)
    assert o.tile_flags(1, 1, 0, 0, True, x_wrap=0) == forced._fused_flags()
    # a north-east rank of a closed 3 x 3 grid: open south and west, both
    # walls; the centre rank: everything open, no wall
    assert o.tile_flags(3, 3, 2, 2, False) == [1, 0, 1, 0, 1, 1, 0]
    assert o.tile_flags(3, 3, 1, 1, False) == [1, 1, 1, 1, 0, 0, 0]
