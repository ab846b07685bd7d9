"""Vertical-line preconditioned CG on the 3-D halo stencil at world 1:
float32 (default) on one field of (64, 1026, 1026), closed edges, periodic
z, the 7-point operator with vertical weight 100 and horizontal weight 1.

Contenders, alternated over several repeats (median with min/max):

* ``cg_iteration`` / ``pcg_iteration``: ``iterate(1)`` of ``make_cg()`` and
  of ``make_cg("zline")`` on the same operator;
* ``fused_update``: ``StencilPCG.update_step`` — one launch of
  ``csrc/zline.hip`` plus two finish launches;
* ``composed_update``: the same result from three steps:
  ``StencilCG.update_step``, ``ZLineSolver.solve`` and ``HaloStencil.dot``;
* ``line_solve``: ``ZLineSolver.solve`` alone; ``copy``: ``z.copy_(r)``, the
  two-stream traffic floor.

``model_pcg_over_cg`` is the traffic prediction 12 / 11 field-sized streams.
Before timing, the fused update is checked against the composition.

``--lds-sweep`` times ``fused_update`` and ``line_solve`` at several
``_lds_planes`` instead.  ``--solve`` also reports time to solution of CG
and PCG on a (64, 258, 258) anisotropic problem (host clock around
``solve`` with ``check_every=8``, ending in the host read).

Run on a GPU box:  python benchmarks/bench_stencil3d_pcg.py [--out r.json]
"""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch  # noqa: E402

import mpi4jax_amd as m  # noqa: E402
from mpi4jax_amd.parallel import CartesianGrid  # noqa: E402
from bench_stencil import _compare  # noqa: E402

SHAPE = (64, 1026, 1026)
SOLVE_SHAPE = (64, 258, 258)


def table(az=100.0):
    k = torch.zeros(3, 3, 3, dtype=torch.float64)
    k[0, 1, 1] = k[2, 1, 1] = -az
    k[1, 0, 1] = k[1, 2, 1] = k[1, 1, 0] = k[1, 1, 2] = -1.0
    k[1, 1, 1] = 1.0 + 2.0 * az + 4.0
    return k


def rhs(shape, dtype):
    torch.manual_seed(7)
    b = torch.zeros(shape, dtype=dtype, device="cuda")
    b[:, 1:-1, 1:-1] = torch.randn(shape[0], shape[1] - 2, shape[2] - 2,
                                   dtype=dtype, device="cuda")
    return b


def started(st, b, lds=None):
    pcg = st.make_cg("zline", _lds_planes=lds)
    pcg.start(b, torch.zeros_like(b))
    pcg.apply_step()  # a pq to divide by
    return pcg


def composed(cg, solver, st, zs, rz):
    cg.update_step()
    solver.solve(*cg._r, out=zs)
    st._dot_into(cg._r, zs, rz)


def case(grid, dtype, run):
    st = grid.make_stencil3d(SHAPE, dtype, "cuda", table(),
                             z_boundary="periodic")
    b = rhs(SHAPE, dtype)
    cg = st.make_cg()
    cg.start(b, torch.zeros_like(b))
    cg.apply_step()
    pcg = started(st, b)
    solver = pcg.line_solver
    zs, rz = [torch.zeros_like(b)], st._scalar()
    # the same update from the same state, both ways
    for dst, src in zip(cg._r + cg._p + cg._q, pcg._r + pcg._p + pcg._q):
        dst.copy_(src)
    cg._rs.copy_(pcg.rz), cg._pq.copy_(pcg.pq)
    pcg.update_step()
    composed(cg, solver, st, zs, rz)
    eps = torch.finfo(dtype).eps
    assert torch.equal(cg._r[0], pcg._r[0])
    assert ((zs[0] - pcg._z[0]).abs().max()
            <= 64 * eps * zs[0].abs().max()), "fused z differs"
    assert abs(rz.item() - pcg.rz.item()) <= 64 * eps * abs(rz.item())
    res = _compare({
        "cg_iteration": lambda: cg.iterate(1),
        "pcg_iteration": lambda: pcg.iterate(1),
        "fused_update": pcg.update_step,
        "composed_update": lambda: composed(cg, solver, st, zs, rz),
        "line_solve": lambda: solver.solve(*pcg._r, out=zs),
        "copy": lambda: zs[0].copy_(b),
    }, *run)
    res["lds_planes"] = solver.lds_planes
    res["model_pcg_over_cg"] = round(12 / 11, 3)
    for num, den in (("pcg_iteration", "cg_iteration"),
                     ("fused_update", "composed_update"),
                     ("line_solve", "copy")):
        res[f"{num}_over_{den}"] = round(
            res[num]["wall_us"] / res[den]["wall_us"], 3)
    return res


def lds_sweep(grid, dtype, run):
    st = grid.make_stencil3d(SHAPE, dtype, "cuda", table(),
                             z_boundary="periodic")
    b = rhs(SHAPE, dtype)
    z = torch.zeros_like(b)
    contenders = {}
    most = st.make_line_solver().lds_planes
    for lds in sorted({0, most // 4, most // 2, most}):
        pcg = started(st, b, lds)
        contenders[f"fused_update_lds{lds}"] = pcg.update_step
        contenders[f"line_solve_lds{lds}"] = (
            lambda s=pcg.line_solver: s.solve(b, out=z))
    return _compare(contenders, *run)


def time_to_solution(grid, dtype):
    st = grid.make_stencil3d(SOLVE_SHAPE, dtype, "cuda", table(),
                             z_boundary="periodic")
    b = rhs(SOLVE_SHAPE, dtype)
    out = {}
    for name, pre in (("cg", None), ("pcg", "zline")):
        solver = st.make_cg(pre)
        solver.solve(b, rtol=1e-5, maxiter=16)  # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, info = solver.solve(b, rtol=1e-5, maxiter=4000)
        out[name] = {"iterations": info.iterations,
                     "converged": info.converged,
                     "wall_ms": round(1e3 * (time.perf_counter() - t0), 2)}
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--float64", action="store_true")
    p.add_argument("--lds-sweep", action="store_true")
    p.add_argument("--solve", action="store_true")
    p.add_argument("--out", default=None,
                   help="also write the JSON result to this file")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stencil3d_pcg.py measures the GPU path; no "
                         "GPU found")
    m.init()
    grid = CartesianGrid(dims=(1, 1), periodic=(False, False))
    dtype = torch.float64 if args.float64 else torch.float32
    run = (args.warmup, args.iters, args.repeats)
    out = {"device": torch.cuda.get_device_name(0), "dtype": str(dtype),
           "shape": SHAPE, "iters": args.iters, "repeats": args.repeats}
    if args.lds_sweep:
        out["lds_sweep"] = lds_sweep(grid, dtype, run)
    else:
        out["iteration"] = case(grid, dtype, run)
    if args.solve:
        out["time_to_solution"] = time_to_solution(grid, dtype)
    print(json.dumps(out, indent=2))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=2)


if __name__ == "__main__":
    main()
