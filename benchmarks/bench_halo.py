"""Halo-exchanger timing at world 1 (periodic in both axes).

(a) three float32 fields (1802, 3602), width 1: the native exchanger
    (2 launches for all three fields) against three calls to
    ``CartesianGrid.halo_exchange_`` on the same tensors, the path the
    library offered before the exchanger existed;
(b) one float32 field (8, 1806, 3606), width 3: the native executor
    against the Python executor of the same exchanger;
(c) ``adjoint_`` (the backward pass of ``exchange_ad``) against
    ``exchange_`` on the same exchanger, for both configurations above.

Per case: wall time per exchange (host clock around a loop that ends in a
device synchronise) and host enqueue time per exchange (a short burst
submitted without waiting), measured as in bench_step_overhead.py.  The
two contenders of a case alternate over several repeats; the median is
reported next to min/max so the spread is visible.  Before timing, the
contenders are checked to produce bitwise-identical fields.

Run on a GPU box:  python benchmarks/bench_halo.py [--out result.json]
``--profile-a N`` runs only N native exchanges of case (a) after a
warm-up — the body of a ``rocprofv3 --kernel-trace --stats`` run;
``--profile-c N`` does the same for the adjoint of that configuration
(besides the warm-up, the run holds the one exchange and one adjoint of
the dot-product check).
"""

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch  # noqa: E402

import mpi4jax_amd as m  # noqa: E402
from mpi4jax_amd.parallel import CartesianGrid  # noqa: E402


def _time(fn, iters, burst):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    wall_us = (time.perf_counter() - t0) / iters * 1e6
    t0 = time.perf_counter()
    for _ in range(burst):
        fn()
    host_us = (time.perf_counter() - t0) / burst * 1e6
    torch.cuda.synchronize()
    return wall_us, host_us


def _compare(contenders, warmup, iters, burst, repeats):
    for fn in contenders.values():
        for _ in range(warmup):
            fn()
    samples = {k: [] for k in contenders}
    for _ in range(repeats):  # alternate the contenders
        for k, fn in contenders.items():
            samples[k].append(_time(fn, iters, burst))
    out = {}
    for k, s in samples.items():
        wall = [a for a, _ in s]
        host = [b for _, b in s]
        out[k] = {
            "wall_us_per_exchange": round(statistics.median(wall), 2),
            "wall_us_min_max": [round(min(wall), 2), round(max(wall), 2)],
            "host_enqueue_us_per_exchange":
                round(statistics.median(host), 2),
            "host_us_min_max": [round(min(host), 2), round(max(host), 2)],
        }
    return out


def _python_executor(ex, fields):
    def run():
        os.environ["MPI4JAX_AMD_HALO_PY"] = "1"
        try:
            ex.exchange_(*fields)
        finally:
            del os.environ["MPI4JAX_AMD_HALO_PY"]
    return run


def case_a(grid, check=True):
    shape = (1802, 3602)
    torch.manual_seed(0)
    fields = [torch.randn(shape, device="cuda") for _ in range(3)]
    ex = grid.make_halo_exchanger(shape, torch.float32, "cuda", width=1,
                                  nfields=3)
    if check:  # same result first
        ref = [grid.halo_exchange(f) for f in fields]
        got = ex.exchange(*fields)
        assert all(torch.equal(a, b) for a, b in zip(ref, got))

    def baseline():
        for f in fields:
            grid.halo_exchange_(f)

    return ex, fields, {"native_exchanger": lambda: ex.exchange_(*fields),
                        "halo_exchange_x3": baseline}


def case_b(grid):
    shape = (8, 1806, 3606)
    torch.manual_seed(1)
    f = torch.randn(shape, device="cuda")
    ex = grid.make_halo_exchanger(shape, torch.float32, "cuda", width=3)
    py = _python_executor(ex, [f])
    a = ex.exchange(f)
    g = f.clone()
    _python_executor(ex, [g])()
    assert torch.equal(a, g)
    return {"native_executor": lambda: ex.exchange_(f),
            "python_executor": py}


def case_c(grid, shape, width, nfields):
    """``adjoint_`` against ``exchange_`` on the same exchanger.  The two
    move the same staging bytes; the adjoint's accumulate kernel visits
    the 2*width-thick frame, about twice the cells of the unpack."""
    torch.manual_seed(2)
    fields = [torch.randn(shape, device="cuda") for _ in range(nfields)]
    ex = grid.make_halo_exchanger(shape, torch.float32, "cuda", width=width,
                                  nfields=nfields)
    # <exchange(x), y> == <x, adjoint(y)> first, in float64 on the host
    ys = [torch.randn(shape, device="cuda") for _ in range(nfields)]
    fx = ex.exchange(*fields)
    ay = ex.adjoint(*ys)
    fx, ay = [(t,) if isinstance(t, torch.Tensor) else t for t in (fx, ay)]
    lhs = sum((a.double() * b.double()).sum().item() for a, b in zip(fx, ys))
    rhs = sum((a.double() * b.double()).sum().item()
              for a, b in zip(fields, ay))
    assert abs(lhs - rhs) <= 1e-5 * max(1.0, abs(lhs)), (lhs, rhs)
    # repeated adjoints of the same tensors grow without bound (each
    # wrap adds a term), so the timed adjoint runs on zeros
    grads = [torch.zeros(shape, device="cuda") for _ in range(nfields)]
    return {"exchange_": lambda: ex.exchange_(*fields),
            "adjoint_": lambda: ex.adjoint_(*grads)}


def _ratio(res):
    res["adjoint_over_exchange_wall"] = round(
        res["adjoint_"]["wall_us_per_exchange"]
        / res["exchange_"]["wall_us_per_exchange"], 3)
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--warmup", type=int, default=50)
    p.add_argument("--iters", type=int, default=2000)
    p.add_argument("--burst", type=int, default=50)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--profile-a", type=int, default=0)
    p.add_argument("--profile-c", type=int, default=0)
    p.add_argument("--cases", default="abc",
                   help="which cases to run, e.g. 'c' (default: all)")
    p.add_argument("--out", default=None,
                   help="also write the JSON result to this file")
    args = p.parse_args()

    if not torch.cuda.is_available():
        raise SystemExit("bench_halo.py measures the GPU path; no GPU found")
    m.init()
    grid = CartesianGrid(dims=(1, 1), periodic=(True, True))

    if args.profile_a:
        ex, fields, _ = case_a(grid, check=False)
        ex.exchange_(*fields)  # warm-up: loads the code object
        torch.cuda.synchronize()
        for _ in range(args.profile_a):
            ex.exchange_(*fields)
        torch.cuda.synchronize()
        print(f"profiled {args.profile_a} native exchanges of case (a)")
        return

    if args.profile_c:
        fns = case_c(grid, (1802, 3602), 1, 3)
        fns["adjoint_"]()  # warm-up: loads the code object
        torch.cuda.synchronize()
        for _ in range(args.profile_c):
            fns["adjoint_"]()
        torch.cuda.synchronize()
        print(f"profiled {args.profile_c} native adjoints of case (c), "
              f"3 x (1802, 3602)")
        return

    out = {"device": torch.cuda.get_device_name(0),
           "iters": args.iters, "repeats": args.repeats}
    run = (args.warmup, args.iters, args.burst, args.repeats)
    if "a" in args.cases:
        out["a_3xf32_1802x3602_w1"] = _compare(case_a(grid)[2], *run)
    if "b" in args.cases:
        out["b_1xf32_8x1806x3606_w3"] = _compare(case_b(grid), *run)
    if "c" in args.cases:
        out["c_adjoint_3xf32_1802x3602_w1"] = _ratio(_compare(
            case_c(grid, (1802, 3602), 1, 3), *run))
        out["c_adjoint_1xf32_8x1806x3606_w3"] = _ratio(_compare(
            case_c(grid, (8, 1806, 3606), 3, 1), *run))
    print(json.dumps(out, indent=2))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=2)


if __name__ == "__main__":
    main()
