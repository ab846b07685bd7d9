"""Chebyshev iteration timing at world 1 (periodic in both axes).

Time per iteration of ``StencilChebyshev.iterate`` — eager, and replayed
from a ``torch.cuda.graph`` — against ``StencilCG.iterate`` and against
the Chebyshev iteration a user composes from ``HaloStencil.apply`` and
torch ops, for the operator ``I - nu * lap`` with the 5-point Laplacian,
float32 and float64, at the two sizes of bench_stencil_cg.py:

* ``small``  one (1, 130, 130) field: the time is launches (1 fused, 5 of
  conjugate gradients, 5 composed);
* ``large``  one (8, 2050, 4098) field, 256 MiB in float32 and 512 MiB in
  float64: past the last-level cache, so the time is memory traffic.  The
  fused step moves 6 field-sized streams (reads d, x, r; writes x, r, d'),
  conjugate gradients 11, the composed step 13; ``streams_GBps`` is each
  contender's own byte count over its measured time, an end-to-end rate
  and not a kernel's share of peak.

The composed baseline is what the library offered before
``make_chebyshev``: ``apply(d, out=q)``, then ``x += d``, ``r -= q``,
``d *= c1`` and ``d += c2 * r`` in place on the strided interior views (no
temporaries, coefficients as Python floats).  It computes what the fused
step computes but for the rounding of ``c1 d + c2 r``.

Then time to tolerance: ``solve`` to ``rtol = 1e-6`` for ``nu`` in
{1, 100}, Chebyshev with Gershgorin's bounds and its a-priori count
(``check_every=0``: no inner product, no host read) against conjugate
gradients with the default test every 8 iterations.  Chebyshev needs more
iterations, each cheaper; the true relative residual of both results is
recorded.

Method as in bench_stencil_cg.py: wall time (host clock around a loop
that ends in a device synchronise) of a block of K iterations, divided by
K; every block starts from ``start(b, 0)`` outside the timed window; the
contenders alternate over several repeats after a warm-up; the median is
reported with min and max.  Before timing, a replayed block is checked
bitwise against an eager one, and the composed iteration against the
fused one.

Run on a GPU box:
    python benchmarks/bench_stencil_chebyshev.py [--out result.json]
"""

import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch  # noqa: E402

import mpi4jax_amd as m  # noqa: E402
from mpi4jax_amd.parallel import CartesianGrid  # noqa: E402

W = 1
NU = 100.0
SIZES = {"small": (1, 130, 130), "large": (8, 2050, 4098)}
# field-sized reads + writes of one iteration
STREAMS = {"cheb": 6, "cg": 11, "composed": 13}
NAMES = ("cheb_eager", "cheb_graph", "cg_eager", "cg_graph",
         "composed_eager", "composed_graph")


def weights(nu):
    k = torch.zeros(3, 3, dtype=torch.float64)
    k[1, 0] = k[1, 2] = k[0, 1] = k[2, 1] = -nu
    k[1, 1] = 1.0 + 4.0 * nu
    return k


def inner(t):
    return t[..., W:-W, W:-W]


def rhs(shape, dtype):
    torch.manual_seed(0)
    b = torch.zeros(shape, dtype=dtype, device="cuda")
    inner(b).copy_(torch.randn(shape[0], shape[1] - 2 * W,
                               shape[2] - 2 * W, device="cuda"))
    return b


class Composed:
    """The same recurrence from ``apply`` and torch ops (module
    docstring); ``coef`` is the fused solver, asked for the scalars."""

    def __init__(self, st, coef, shape, dtype):
        self.st, self.coef = st, coef
        z = dict(dtype=dtype, device="cuda")
        self.x, self.r = torch.zeros(shape, **z), torch.zeros(shape, **z)
        self.d, self.q = torch.zeros(shape, **z), torch.zeros(shape, **z)
        self.k = 0

    def start(self, b, x=None):
        self.x.zero_()
        inner(self.r).copy_(inner(b))
        torch.div(inner(b), self.coef.theta, out=inner(self.d))
        self.k = 0

    def iterate(self, n):
        x, r, d, q = self.x, self.r, self.d, self.q
        for _ in range(n):
            c1, c2 = self.coef.coefficients(self.k)
            self.st.apply(d, out=q)
            inner(x).add_(inner(d))
            inner(r).sub_(inner(q))
            inner(d).mul_(c1).add_(inner(r), alpha=c2)
            self.k += 1


class Case:
    def __init__(self, grid, size, dtype, block):
        shape = SIZES[size]
        self.shape, self.dtype, self.block = shape, dtype, block
        self.st = grid.make_stencil(shape, dtype, "cuda", weights(NU))
        self.bounds = self.st.gershgorin_bounds()
        self.b = rhs(shape, dtype)
        self.solver, self.x, self.graph = {}, {}, {}
        for name in NAMES:
            kind = name.split("_")[0]
            if kind == "cheb":
                s = self.st.make_chebyshev(*self.bounds)
            elif kind == "cg":
                s = self.st.make_cg()
            else:
                s = Composed(self.st, self.solver["cheb_eager"], shape,
                             dtype)
            self.solver[name] = s
            self.x[name] = (s.x if kind == "composed"
                            else torch.zeros_like(self.b))

    def _restart(self, name):
        self.x[name].zero_()
        self.solver[name].start(self.b, self.x[name])

    def _capture(self, name):
        s = self.solver[name]
        self._restart(name)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            s.iterate(self.block)  # warm-up on a side stream
        torch.cuda.current_stream().wait_stream(side)
        self._restart(name)  # the graph holds the coefficients from k = 0
        self.graph[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph[name]):
            s.iterate(self.block)

    def run(self, name):
        """One block of ``block`` iterations, enqueued."""
        if name.endswith("_graph"):
            self.graph[name].replay()
        else:
            self.solver[name].iterate(self.block)

    def check(self, few=5):
        """A replay is the eager sequence, bitwise; the composed step
        rounds ``c1 d + c2 r`` differently, so it is compared with the
        fused one after ``few`` iterations."""
        for name in NAMES:
            if name.endswith("_graph"):
                self._capture(name)
        for name in NAMES:
            self._restart(name)
            self.run(name)
        torch.cuda.synchronize()
        for kind in ("cheb", "cg", "composed"):
            assert torch.equal(self.x[kind + "_eager"],
                               self.x[kind + "_graph"]), \
                f"{kind}: graph replay != eager"
        self._restart("cheb_eager")
        self._restart("composed_eager")
        self.solver["cheb_eager"].iterate(few)
        self.solver["composed_eager"].iterate(few)
        ref = inner(self.x["cheb_eager"]).double()
        rel = ((inner(self.x["composed_eager"]).double() - ref).norm()
               / ref.norm()).item()
        tol = 1e-4 if self.dtype == torch.float32 else 1e-11
        assert rel < tol, f"composed iteration differs by {rel:.2e}"
        return {"composed_vs_fused_rel_diff": rel, "after": few}

    def time_block(self, name):
        self._restart(name)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.run(name)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / self.block * 1e6


def time_to_tolerance(grid, size, dtype, nu, rtol, repeats):
    """Wall time of a whole ``solve`` (start included, result
    synchronised), median of ``repeats`` after one warm-up."""
    shape = SIZES[size]
    st = grid.make_stencil(shape, dtype, "cuda", weights(nu))
    b = rhs(shape, dtype)
    cheb = st.make_chebyshev(*st.gershgorin_bounds())
    cg = st.make_cg()
    check = torch.zeros_like(b)
    bnorm = math.sqrt(st.dot(b, b).item())

    def true_residual(x):
        st.apply(x, out=check)
        check.sub_(b)
        return math.sqrt(st.dot(check, check).item()) / bnorm

    def timed(fn):
        samples = []
        for i in range(repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            x, info = fn()
            torch.cuda.synchronize()
            if i:
                samples.append((time.perf_counter() - t0) * 1e3)
        return x, info, samples

    out = {"shape": list(shape), "nu": nu, "rtol": rtol, "unit": "ms"}
    x, info, s = timed(lambda: cheb.solve(b, rtol=rtol, check_every=0))
    out["chebyshev"] = {
        "ms": round(statistics.median(s), 3),
        "ms_min_max": [round(min(s), 3), round(max(s), 3)],
        "iterations": info.iterations,
        "true_rel_residual": true_residual(x)}
    x, info, s = timed(lambda: cg.solve(b, rtol=rtol, maxiter=1000))
    out["cg"] = {
        "ms": round(statistics.median(s), 3),
        "ms_min_max": [round(min(s), 3), round(max(s), 3)],
        "iterations": info.iterations, "converged": info.converged,
        "true_rel_residual": true_residual(x)}
    out["cg_over_chebyshev"] = round(out["cg"]["ms"]
                                     / out["chebyshev"]["ms"], 3)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--warmup", type=int, default=3,
                   help="untimed blocks per contender")
    p.add_argument("--repeats", type=int, default=9)
    p.add_argument("--block-small", type=int, default=200,
                   help="iterations per timed block of the small size")
    p.add_argument("--block-large", type=int, default=40)
    p.add_argument("--sizes", default="small,large")
    p.add_argument("--solve-repeats", type=int, default=3)
    p.add_argument("--out", default=None,
                   help="also write the JSON result to this file")
    args = p.parse_args()

    if not torch.cuda.is_available():
        raise SystemExit("bench_stencil_chebyshev.py measures the GPU "
                         "path; no GPU found")
    m.init()
    grid = CartesianGrid(dims=(1, 1), periodic=(True, True))
    out = {"device": torch.cuda.get_device_name(0),
           "repeats": args.repeats, "unit": "us per iteration",
           "streams": STREAMS}
    for size in args.sizes.split(","):
        block = args.block_small if size == "small" else args.block_large
        for dtype in (torch.float32, torch.float64):
            case = Case(grid, size, dtype, block)
            res = {"shape": list(SIZES[size]), "block": block,
                   "bounds": list(case.bounds), "check": case.check()}
            for name in NAMES:
                for _ in range(args.warmup):
                    case.time_block(name)
            samples = {k: [] for k in NAMES}
            for _ in range(args.repeats):  # alternate the contenders
                for name in NAMES:
                    samples[name].append(case.time_block(name))
            field = case.b.numel() * case.b.element_size()
            for k, s in samples.items():
                med = statistics.median(s)
                nbytes = STREAMS[k.split("_")[0]] * field
                res[k] = {"us": round(med, 2),
                          "us_min_max": [round(min(s), 2), round(max(s), 2)],
                          "streams_GBps": round(nbytes / med / 1e3, 1)}
            for mode in ("eager", "graph"):
                for other in ("composed", "cg"):
                    res[f"{other}_over_cheb_{mode}"] = round(
                        res[f"{other}_{mode}"]["us"]
                        / res[f"cheb_{mode}"]["us"], 3)
            out[f"{size}_{str(dtype).split('.')[-1]}"] = res
            del case
            torch.cuda.empty_cache()
    solves = []
    for size in args.sizes.split(","):
        for dtype in (torch.float32, torch.float64):
            for nu in (1.0, 100.0):
                r = time_to_tolerance(grid, size, dtype, nu, 1e-6,
                                      args.solve_repeats)
                r["size"], r["dtype"] = size, str(dtype).split(".")[-1]
                solves.append(r)
                torch.cuda.empty_cache()
    out["time_to_rtol_1e-6"] = solves
    print(json.dumps(out, indent=2))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=2)


if __name__ == "__main__":
    main()
