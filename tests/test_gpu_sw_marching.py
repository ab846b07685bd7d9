"""The march of the single-launch world-1 shallow-water step (stage 30/31,
kernel ``sw_step1t``): a block owns up to K consecutive fast tiles of one
tile column, keeps the 4 window rows and 2 fill rows that neighbouring
tiles share in LDS and prefetches the next tile's 14 new window rows.

K is a runtime value of one binary (``MPI4JAX_AMD_SW_MARCH``, the optional
8th entry of ``sw_stage``'s flags), and every pair goes through the same
compiled fill and friction bodies whatever K is, so every K must give the
same bits.  K = 1 is the schedule without a march (one tile per block,
nothing carried), which the existing tests hold against the three-launch
form, the two-kernel path and the float64 oracle.

Shapes are (nx, ny) as in ``test_gpu_sw_staged_tile.py``, whose docstring
derives which tiles are fast: tile rows 1 <= tr with 14*tr + 15 <= ny and
tile columns 1 <= tc with 60*tc + 62 <= nx.

* (185, 43): tr, tc in {1, 2}: the shortest column that can march, 2 tiles;
* (122, 85): one fast tile column, tr = 1..5; K = 2 splits it 2, 2, 1;
* (250, 100): tr = 1..6, tc = 1..3.

K = 64 is longer than any of these columns: one segment per column.  The
host test runs the enumeration that kernel and launcher share
(``csrc/sw_tiles.h``) through a small C++ program.
"""

import functools
import os
import pathlib
import subprocess

import pytest
import torch

import mpi4jax_amd as m

REPO = pathlib.Path(__file__).resolve().parent.parent
FIELDS = ("h", "u", "v", "dh", "du", "dv")
ENVS = ("MPI4JAX_AMD_SW_RING3", "MPI4JAX_AMD_SW_NOFUSE",
        "MPI4JAX_AMD_SW_FUSE512", "MPI4JAX_AMD_SW_GRAPH",
        "MPI4JAX_AMD_SW_MARCH")
SHAPES = [(185, 43), (122, 85), (250, 100)]
MARCHES = [None, "2", "3", "64"]  # None = unset, the launcher's default
# (nx, ny) -> fast tile rows and columns (first, last), from the docstring
FAST = {(185, 43): ((1, 2), (1, 2)), (122, 85): ((1, 5), (1, 1)),
        (250, 100): ((1, 6), (1, 3)), (3600, 1800): ((1, 127), (1, 58))}


@pytest.fixture(scope="module")
def gpu_world():
    m.init()
    yield
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def _trajectory(nx, ny, periodic, march, stage):
    """(state after the Euler step, state after 8 more steps), computed
    once per case and shared between the tests."""
    from mpi4jax_amd.models import ShallowWater

    with pytest.MonkeyPatch.context() as mp:
        for k in ENVS:
            mp.delenv(k, raising=False)
        if march is not None:
            mp.setenv("MPI4JAX_AMD_SW_MARCH", march)
        if stage == 31:
            mp.setenv("MPI4JAX_AMD_SW_FUSE512", "1")
        sw = ShallowWater(nx=nx, ny=ny, device="cuda", fused=True,
                          periodic_x=periodic, comm=m.get_world().Clone())
        assert sw._stage_plan()[1] == stage
        assert len(sw._fused_flags()) == (7 if march is None else 8)
        st = sw.step(sw.initial_conditions(), first_step=True)
        torch.cuda.synchronize()
        # the model double-buffers in place: snapshot by value
        first = {k: getattr(st, k).clone() for k in FIELDS}
        for _ in range(8):
            st = sw.step(st)
        torch.cuda.synchronize()
        return first, {k: getattr(st, k).clone() for k in FIELDS}


def _assert_bitwise(nx, ny, periodic, march, stage):
    ref = _trajectory(nx, ny, periodic, "1", stage)
    new = _trajectory(nx, ny, periodic, march, stage)
    for i, step in enumerate(("step1", "step9")):
        for name in FIELDS:
            a, b = ref[i][name], new[i][name]
            assert a.shape == (ny + 2, nx + 2)
            assert torch.isfinite(a).all(), (step, name, "non-finite")
            d = (a - b).abs().max().item()
            assert torch.equal(a, b), (step, name, d)


@pytest.mark.gpu
@pytest.mark.parametrize("march", MARCHES)
@pytest.mark.parametrize("periodic", [True, False])
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_march_length_does_not_change_a_bit(gpu_world, nx, ny, periodic,
                                            march):
    _assert_bitwise(nx, ny, periodic, march, 30)


@pytest.mark.gpu
@pytest.mark.parametrize("march", MARCHES)
def test_march_length_does_not_change_a_bit_512_threads(gpu_world, march):
    _assert_bitwise(185, 43, False, march, 31)


# ---------------------------------------------------------------- host


@pytest.fixture(scope="module")
def enum_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("sw_tiles") / "sw_tiles_enum"
    subprocess.run(
        [os.environ.get("CXX", "c++"), "-std=c++17", "-O1",
         f"-I{REPO / 'mpi4jax_amd' / 'csrc'}",
         str(REPO / "tests" / "sw_tiles_enum.cpp"), "-o", str(exe)],
        check=True, capture_output=True, text=True, timeout=120)
    return exe


def _enumerate(exe, nx, ny, periodic, march):
    out = subprocess.run(
        [str(exe), str(ny + 2), str(nx + 2), str(int(periodic)), str(march)],
        check=True, capture_output=True, text=True, timeout=60).stdout
    lines = out.split("\n")
    head = [int(x) for x in lines[0].split()[1:]]
    blocks = [tuple(int(x) for x in ln.split()) for ln in lines[1:] if ln]
    return head, blocks


@pytest.mark.parametrize("periodic", [True, False])
@pytest.mark.parametrize("nx,ny", SHAPES + [(3600, 1800)])
def test_segments_cover_every_fast_tile_once(enum_program, nx, ny, periodic):
    (r0, r1), (c0, c1) = FAST[(nx, ny)]
    base_head, base = _enumerate(enum_program, nx, ny, periodic, 1)
    base_perim = [b for b in base if b[1] != 2]
    for march in (1, 2, 3, 6, 64):
        head, blocks = _enumerate(enum_program, nx, ny, periodic, march)
        grid, tr0, tr1, tc0, tc1, nper, nper_pad, nseg = head
        assert (tr0, tr1, tc0, tc1) == (r0, r1, c0, c1)
        assert grid == nper_pad + nseg == len(blocks)
        assert [b[0] for b in blocks] == list(range(grid))
        # perimeter and padding blocks: the lowest ids, as without a march
        assert [b for b in blocks if b[1] != 2] == base_perim
        assert blocks[:nper_pad] == base_perim and nper_pad % 8 == 0
        assert head[5:7] == base_head[5:7]
        owners = {}
        lengths = {}
        for _, flavour, tr, tc, nt in blocks[nper_pad:]:
            assert flavour == 2 and 1 <= nt <= march
            lengths.setdefault(tc, []).append(nt)
            for r in range(tr, tr + nt):
                assert (r, tc) not in owners, (march, r, tc)
                owners[(r, tc)] = 1
        assert set(owners) == {(r, c) for r in range(r0, r1 + 1)
                               for c in range(c0, c1 + 1)}
        rows = r1 - r0 + 1
        for tc, ls in lengths.items():
            assert max(ls) - min(ls) <= 1, (march, tc, ls)
            assert len(ls) == -(-rows // march), (march, tc, ls)
        # no perimeter tile is a fast tile
        for _, flavour, tr, tc, nt in blocks[:nper_pad]:
            assert flavour == 0 or ((tr, tc) not in owners and nt == 1)
        if march == 1:
            assert nseg == rows * (c1 - c0 + 1)
        if (nx, ny, march) == (122, 85, 2):
            assert sorted(lengths[1], reverse=True) == [2, 2, 1]
