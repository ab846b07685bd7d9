"""Per-column tridiagonal solves at world 1: ``ColumnTridiagonal.solve``
(prefactored) and ``solve_bands`` (factorise and solve in one launch) at
every ``rhs_per_thread``, next to the Python executor on the same device.

Shape: an ocean-like column count, nz = 64 over a 512 x 512 interior
(halo width 1), with 1 and 4 right-hand sides (batch columns of one
field).  Bands are diagonally dominant and in the field dtype.

Streams.  A field-sized stream is ``nz * 512 * 512`` values.  With ``G =
ceil(nrhs / R)`` groups of right-hand sides the least a launch can move is

* ``solve``: ``2 nrhs + 3 G`` streams (r in, x out; inv, lo, cp per group);
* ``solve_bands``: ``2 nrhs + 3 G`` as well (lower, diag, upper per group),

and ``ideal_GBps`` is those bytes over the measured time: what the launch
achieves against its own least traffic.  The planes that do not fit in LDS
add a write and a read of y per right-hand side (and of cp per group on
the fused path); ``moved_GBps`` counts those too.  The contenders are
alternated over several repeats (median with min/max); before timing every
``R`` is checked bitwise against ``R = 1`` and the Python executor against
it to rounding.

Run on a GPU box:  python benchmarks/bench_ztridiag.py [--out r.json]
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch  # noqa: E402

import mpi4jax_amd as m  # noqa: E402
from mpi4jax_amd.parallel import CartesianGrid  # noqa: E402
from bench_stencil import _compare  # noqa: E402

NZ, N, W = 64, 512, 1


def bands(dtype):
    g = torch.Generator().manual_seed(1)
    shape = (NZ, N + 2 * W, N + 2 * W)
    lower, upper, extra = (torch.rand(shape, generator=g, dtype=torch.float64)
                           for _ in range(3))
    lower, upper = -(0.2 + 0.8 * lower), -(0.2 + 0.8 * upper)
    diag = lower.abs() + upper.abs() + 0.1 + 0.9 * extra
    return tuple(b.to(dtype).cuda() for b in (lower, diag, upper))


def python_executor(fn):
    def run():
        os.environ["MPI4JAX_AMD_HALO_PY"] = "1"
        try:
            return fn()
        finally:
            del os.environ["MPI4JAX_AMD_HALO_PY"]
    return run


def case(grid, nrhs, dtype, run):
    shape = (nrhs, NZ, N + 2 * W, N + 2 * W)
    bd = bands(dtype)
    g = torch.Generator().manual_seed(2)
    r = torch.randn(shape, generator=g).to(dtype).cuda()
    out = torch.zeros_like(r)
    stream = NZ * N * N * r.element_size()
    contenders, info, first = {}, {}, None
    for rpt in (1, 2, 4):
        ts = grid.make_tridiagonal_solver(shape, dtype, "cuda", *bd, width=W,
                                          _rhs_per_thread=rpt)
        x, xb = ts.solve(r), ts.solve_bands(*bd, r)
        assert torch.equal(x, xb), "solve_bands differs from solve"
        if first is None:
            first = x
            py = python_executor(lambda: ts.solve(r))()
            # |T|_inf <= 5 and |T^-1|_inf <= 1 / 0.1: kappa_inf <= 50
            eps = torch.finfo(dtype).eps
            assert (py - x).abs().max() <= 16 * 50 * eps * x.abs().max()
            contenders["solve_python"] = python_executor(
                lambda s=ts: s.solve(r, out=out))
            contenders["solve_bands_python"] = python_executor(
                lambda s=ts: s.solve_bands(*bd, r, out=out))
        assert torch.equal(x, first), "the result depends on R"
        groups = -(-nrhs // rpt)
        for name, fn, lds, slots in (
                ("solve", lambda s=ts: s.solve(r, out=out), ts.lds_planes,
                 0),
                ("solve_bands", lambda s=ts: s.solve_bands(*bd, r, out=out),
                 ts._lds_fused, 1)):
            key = f"{name}_R{rpt}"
            contenders[key] = fn
            spilled = (NZ - lds) / NZ * 2 * (nrhs + slots * groups)
            info[key] = {"lds_planes": lds,
                         "ideal_streams": 2 * nrhs + 3 * groups,
                         "moved_streams": round(
                             2 * nrhs + 3 * groups + spilled, 2)}
    res = _compare(contenders, *run)
    for key, extra in info.items():
        sec = res[key]["wall_us"] * 1e-6
        res[key].update(extra)
        res[key]["ideal_GBps"] = round(
            extra["ideal_streams"] * stream / sec / 1e9, 1)
        res[key]["moved_GBps"] = round(
            extra["moved_streams"] * stream / sec / 1e9, 1)
    for name in ("solve", "solve_bands"):
        res[f"{name}_python"]["ideal_GBps"] = round(
            5 * nrhs * stream / (res[f"{name}_python"]["wall_us"] * 1e-6)
            / 1e9, 1)
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--float64", action="store_true")
    p.add_argument("--out", default=None,
                   help="also write the JSON result to this file")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ztridiag.py measures the GPU path; no GPU "
                         "found")
    m.init()
    grid = CartesianGrid(dims=(1, 1), periodic=(False, False))
    dtype = torch.float64 if args.float64 else torch.float32
    run = (args.warmup, args.iters, args.repeats)
    out = {"device": torch.cuda.get_device_name(0), "dtype": str(dtype),
           "shape": [NZ, N + 2 * W, N + 2 * W], "width": W,
           "iters": args.iters, "repeats": args.repeats, "nrhs": {}}
    for nrhs in (1, 4):
        out["nrhs"][str(nrhs)] = case(grid, nrhs, dtype, run)
    print(json.dumps(out, indent=2))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=2)


if __name__ == "__main__":
    main()
