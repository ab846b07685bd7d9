"""Line solve and fused PCG update at world 1, ``method="thomas"`` against
``"pcr"``: float32, periodic z, closed edges, the operator of
bench_stencil3d_pcg.py (vertical weight 100, horizontal 1).

Shapes: interiors of 16^2, 32^2, 64^2 and 256^2 at nz = 64 and 128, the
small horizontal blocks with tall columns that ``"pcr"`` is for, and the
(64, 1026, 1026) of bench_stencil3d_pcg.py, where both are bound by memory
traffic.  Per shape the four contenders are alternated over several repeats
(median with min/max):

* ``line_solve_thomas`` / ``line_solve_pcr``: ``ZLineSolver.solve``;
* ``fused_update_thomas`` / ``fused_update_pcr``:
  ``StencilPCG.update_step``, one launch plus two finish launches.

``pcr_over_thomas`` is the ratio of the medians and ``ranges_overlap`` says
whether the min..max ranges of the two meet.  Before timing, the two
methods' solves are checked against each other.

Run on a GPU box:  python benchmarks/bench_zline_pcr.py [--out r.json]
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
from bench_stencil3d_pcg import SHAPE, rhs, table  # noqa: E402

SMALL = [(nz, n + 2, n + 2) for n in (16, 32, 64, 256) for nz in (64, 128)]


def case(grid, shape, dtype, run):
    st = grid.make_stencil3d(shape, dtype, "cuda", table(),
                             z_boundary="periodic")
    b = rhs(shape, dtype)
    contenders, z, res = {}, {}, {}
    for method in ("thomas", "pcr"):
        pcg = st.make_cg("zline", line_method=method)
        pcg.start(b, torch.zeros_like(b))
        pcg.apply_step()  # a pq to divide by
        solver = pcg.line_solver
        z[method] = solver.solve(b)
        out = [torch.zeros_like(b)]
        contenders[f"line_solve_{method}"] = (
            lambda s=solver, o=out: s.solve(b, out=o))
        contenders[f"fused_update_{method}"] = pcg.update_step
        if method == "pcr":
            res["columns_per_block"] = solver.columns_per_block
            res["levels"] = solver.levels
    # kappa_inf(T) = 405 / 5: each is within 16 eps kappa of the solution
    eps = torch.finfo(dtype).eps
    assert ((z["pcr"] - z["thomas"]).abs().max()
            <= 32 * 81 * eps * z["thomas"].abs().max()), "the methods differ"
    res.update(_compare(contenders, *run))
    for what in ("line_solve", "fused_update"):
        pcr, thomas = res[f"{what}_pcr"], res[f"{what}_thomas"]
        lo, hi = pcr["wall_us_min_max"], thomas["wall_us_min_max"]
        res[what] = {
            "pcr_over_thomas": round(pcr["wall_us"] / thomas["wall_us"], 3),
            "ranges_overlap": not (lo[1] < hi[0] or hi[1] < lo[0])}
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--float64", action="store_true")
    p.add_argument("--skip-large", action="store_true",
                   help="leave out the (64, 1026, 1026) shape")
    p.add_argument("--out", default=None,
                   help="also write the JSON result to this file")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_zline_pcr.py measures the GPU path; no GPU "
                         "found")
    m.init()
    grid = CartesianGrid(dims=(1, 1), periodic=(False, False))
    dtype = torch.float64 if args.float64 else torch.float32
    run = (args.warmup, args.iters, args.repeats)
    out = {"device": torch.cuda.get_device_name(0), "dtype": str(dtype),
           "iters": args.iters, "repeats": args.repeats, "shapes": {}}
    for shape in SMALL + ([] if args.skip_large else [SHAPE]):
        out["shapes"]["x".join(map(str, shape))] = case(grid, shape, dtype,
                                                        run)
    print(json.dumps(out, indent=2))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=2)


if __name__ == "__main__":
    main()
