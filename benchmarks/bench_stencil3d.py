"""3-D halo stencil timing at world 1 (periodic in y and x, zero z
boundary): the 7-point star and the 27-point box, float32 and float64, one
field of (256, 258, 258) and of (64, 1026, 1026).

Contenders of a case:

* ``apply``: ``HaloStencil3D.apply(u, out=v)`` with the host's z-chunk
  rule; ``apply_zc1`` forces one output plane per block;
* ``python``: the Python executor on the GPU (``exchange`` plus one torch
  slicing multiply-add per tap), the only way to this result before;
* ``copy``: ``v.copy_(u)``, the two-stream traffic floor;
* ``flat``: a 2-D ``HaloStencil.apply`` with the in-plane taps of the same
  table (5 or 9) on the same array: what the kernel without z coupling
  costs.  Not a correctness peer;
* ``cg_iteration`` (star only): one ``StencilCG.iterate(1)`` on the 3-D
  operator.

``model_apply_over_flat`` is the chunk redundancy ``(zc + 2 rz) / zc`` of
input planes read per output plane.

Per contender: wall time per call (host clock around a loop that ends in a
device synchronise).  The contenders of a case alternate over several
repeats; the median is reported with min/max so the spread is visible.
Before timing, ``apply`` is checked against ``python``.

``--zc-sweep`` times the star's ``apply`` at every power-of-two z chunk
instead, next to the host's choice.  ``--profile N`` is the body of a
profiler run: N calls each of the star's ``apply`` and ``flat`` in float32
at (64, 1026, 1026), nothing timed.

Run on a GPU box:  python benchmarks/bench_stencil3d.py [--out r.json]
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

SHAPES = [(256, 258, 258), (64, 1026, 1026)]


def table(kind):
    k = torch.full((3, 3, 3), -0.03125, dtype=torch.float64)
    if kind == "star7":
        k.zero_()
        for o in ((0, 1, 1), (2, 1, 1), (1, 0, 1), (1, 2, 1), (1, 1, 0),
                  (1, 1, 2)):
            k[o] = -0.125
    k[1, 1, 1] = 2.0  # diagonally dominant: CG's operator is SPD
    return k


def case(grid, kind, dtype, shape, run):
    k = table(kind)
    torch.manual_seed(len(kind))
    u = torch.randn(shape, dtype=dtype, device="cuda")
    u[:, :1].zero_(), u[:, -1:].zero_(), u[..., :1].zero_(), u[..., -1:].zero_()
    v, s = torch.zeros_like(u), torch.zeros_like(u)
    st = grid.make_stencil3d(shape, dtype, "cuda", k)
    st1 = grid.make_stencil3d(shape, dtype, "cuda", k, _z_chunk=1)
    flat = grid.make_stencil(shape, dtype, "cuda", k[1])
    contenders = {
        "apply": lambda: st.apply(u, out=v),
        "apply_zc1": lambda: st1.apply(u, out=v),
        "python": lambda: st._apply_py((u,), (s,)),
        "copy": lambda: v.copy_(u),
        "flat": lambda: flat.apply(u, out=v),
    }
    if kind == "star7":
        cg = st.make_cg()
        cg.start(u, torch.zeros_like(u))
        contenders["cg_iteration"] = lambda: cg.iterate(1)
    contenders["apply"]()
    contenders["python"]()
    err = (v.double() - s.double()).abs().max().item()
    tol = 27 * 4 * (2.0 ** -24 if dtype == torch.float32 else 2.0 ** -53)
    assert err <= tol * 2.0 * u.abs().max().item(), (kind, dtype, shape, err)
    res = _compare(contenders, *run)
    zc = st.z_chunk
    res["z_chunk"] = zc
    res["model_apply_over_flat"] = round((zc + 2) / zc, 3)
    for num, den in (("apply", "flat"), ("apply", "copy"),
                     ("python", "apply"), ("apply_zc1", "apply")):
        res[f"{num}_over_{den}"] = round(
            res[num]["wall_us"] / res[den]["wall_us"], 3)
    return res


def sweep(grid, dtype, shape, run):
    """``apply`` of the star at every power-of-two z chunk up to nz."""
    u = torch.randn(shape, dtype=dtype, device="cuda")
    v = torch.zeros_like(u)
    contenders = {}
    zc = 1
    while zc <= shape[0]:
        st = grid.make_stencil3d(shape, dtype, "cuda", table("star7"),
                                 _z_chunk=zc)
        contenders[f"zc{zc}"] = lambda st=st: st.apply(u, out=v)
        zc *= 2
    res = _compare(contenders, *run)
    res["host_choice"] = grid.make_stencil3d(shape, dtype, "cuda",
                                             table("star7")).z_chunk
    return res


def profile(grid, n):
    shape, k = SHAPES[1], table("star7")
    u = torch.randn(shape, device="cuda")
    v = torch.zeros_like(u)
    st = grid.make_stencil3d(shape, torch.float32, "cuda", k)
    flat = grid.make_stencil(shape, torch.float32, "cuda", k[1])
    for _ in range(n):
        st.apply(u, out=v)
        flat.apply(u, out=v)
    torch.cuda.synchronize()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--zc-sweep", action="store_true",
                   help="time the star at every power-of-two z chunk "
                        "instead of the contenders")
    p.add_argument("--profile", type=int, default=0, metavar="N",
                   help="run N calls of apply and flat and exit")
    p.add_argument("--out", default=None,
                   help="also write the JSON result to this file")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stencil3d.py measures the GPU path; no GPU "
                         "found")
    m.init()
    grid = CartesianGrid(dims=(1, 1), periodic=(True, True))
    if args.profile:
        return profile(grid, args.profile)
    out = {"device": torch.cuda.get_device_name(0),
           "gpu_id": os.environ.get("HIP_VISIBLE_DEVICES", "0"),
           "iters": args.iters, "repeats": args.repeats}
    for kind in ("star7", "box27"):
        for dtype in (torch.float32, torch.float64):
            for shape in SHAPES:
                name = f"{kind}_{str(dtype)[6:]}_{shape[0]}x{shape[1]}"
                run = (args.warmup, args.iters, args.repeats)
                if not args.zc_sweep:
                    out[name] = case(grid, kind, dtype, shape, run)
                elif kind == "star7":
                    out[name] = sweep(grid, dtype, shape, run)
                torch.cuda.empty_cache()
    print(json.dumps(out, indent=2))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=2)


if __name__ == "__main__":
    main()
