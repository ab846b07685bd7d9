"""Variable-coefficient halo stencil timing at world 1 (periodic in both
axes): a 5-point and a 9-point operator with one coefficient plane per tap,
float32 and float64, fields of (levels, 1802, 3602) at 1 and 16 levels.

Contenders of a case:

* ``variable``: ``VariableHaloStencil.apply(u, out=v)`` with the host's
  levels-per-block rule; ``variable_lpb1`` and ``variable_lpbL`` force one
  level per block and the whole level range;
* ``constant``: ``HaloStencil.apply`` of the same shape and tap count;
* ``slicing``: ``exchange`` plus one torch slicing multiply-add per tap
  with device coefficient tensors, the path the library offered before.

``model`` is the traffic model next to which the times are to be read:
variable / constant = (2 * lpb + T) / (2 * lpb) field-sized streams.

Per contender: wall time per call (host clock around a loop that ends in a
device synchronise).  The contenders of a case alternate over several
repeats; the median is reported with min/max so the spread is visible.
Before timing, ``variable`` is checked against ``slicing`` in float64.

Run on a GPU box:  python benchmarks/bench_varstencil.py [--out r.json]
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

NY, NX = 1802, 3602
OFFSETS = {5: [(0, 0), (-1, 0), (0, -1), (0, 1), (1, 0)],
           9: [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]}


def case(grid, ntaps, dtype, levels, run):
    offsets, shape = OFFSETS[ntaps], (levels, NY, NX)
    torch.manual_seed(ntaps)
    coef = torch.randn(ntaps, NY, NX, dtype=dtype, device="cuda")
    u = torch.randn(shape, dtype=dtype, device="cuda")
    v = torch.zeros_like(u)

    def variable(lpb=None):
        st = grid.make_variable_stencil(shape, dtype, "cuda", offsets, coef,
                                        _levels_per_block=lpb)
        return st, lambda: st.apply(u, out=v)

    st, auto = variable()
    contenders = {"variable": auto, "variable_lpb1": variable(1)[1]}
    if levels > 1:
        contenders["variable_lpbL"] = variable(levels)[1]
    table = torch.zeros(3, 3, dtype=torch.float64)
    for t, (dy, dx) in enumerate(offsets):
        table[1 + dy, 1 + dx] = 0.1 * (t + 1)
    const = grid.make_stencil(shape, dtype, "cuda", table)
    contenders["constant"] = lambda: const.apply(u, out=v)
    ki = coef[:, 1:-1, 1:-1]
    s = torch.zeros_like(u)

    def slicing():
        e = st.exchanger.exchange(u)
        acc = s[:, 1:-1, 1:-1].zero_()
        for t, (dy, dx) in enumerate(offsets):
            acc += ki[t] * e[:, 1 + dy:NY - 1 + dy, 1 + dx:NX - 1 + dx]

    contenders["slicing"] = slicing
    auto()
    slicing()
    err = (v[:, 1:-1, 1:-1].double() - s[:, 1:-1, 1:-1].double()).abs().max()
    tol = ntaps * 4 * (2.0 ** -24 if dtype == torch.float32 else 2.0 ** -53)
    scale = (coef.abs().max() * u.abs().max()).item()
    assert err.item() <= tol * scale, (ntaps, dtype, levels, err.item())
    res = _compare(contenders, *run)
    lpb = st.levels_per_block
    res["levels_per_block"] = lpb
    res["model_variable_over_constant"] = round(
        (2 * lpb + ntaps) / (2 * lpb), 3)
    res["variable_over_constant"] = round(
        res["variable"]["wall_us"] / res["constant"]["wall_us"], 3)
    res["slicing_over_variable"] = round(
        res["slicing"]["wall_us"] / res["variable"]["wall_us"], 3)
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--iters", type=int, default=30)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--out", default=None,
                   help="also write the JSON result to this file")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_varstencil.py measures the GPU path; no GPU "
                         "found")
    m.init()
    grid = CartesianGrid(dims=(1, 1), periodic=(True, True))
    out = {"device": torch.cuda.get_device_name(0), "iters": args.iters,
           "repeats": args.repeats}
    for ntaps in (5, 9):
        for dtype in (torch.float32, torch.float64):
            for levels in (1, 16):
                name = f"{ntaps}pt_{str(dtype)[6:]}_L{levels}"
                out[name] = case(grid, ntaps, dtype, levels,
                                 (args.warmup, args.iters, args.repeats))
                torch.cuda.empty_cache()
    print(json.dumps(out, indent=2))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=2)


if __name__ == "__main__":
    main()
