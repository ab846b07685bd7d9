"""Conjugate-gradient iteration timing at world 1 (periodic in both axes).

Time per iteration of ``StencilCG.iterate`` — eager, and replayed from a
``torch.cuda.graph`` — against the iteration a user composes from
``HaloStencil.apply`` and torch ops, for the operator ``I - nu * lap`` with
the 5-point Laplacian, float32 and float64, at two sizes:

* ``small``  one (1, 130, 130) field: every kernel is far below a
  microsecond of traffic, so the time is launches (5 native, 10 composed);
* ``large``  one (8, 2050, 4098) field, 256 MiB in float32 and 512 MiB in
  float64: past the last-level cache, so the time is memory traffic.  The
  native iteration moves 11 field-sized streams (apply_dot reads p and
  writes q; the update reads x, p, r, q and writes x, r; the direction
  reads r, p and writes p); ``streams_GBps`` is that byte count over the
  measured time, an end-to-end rate and not a kernel's share of peak.

The composed baseline is kept here so that the comparison can be repeated.
It is what the library offered before ``make_cg``, written the way a
careful user would: ``alpha`` and ``beta`` stay device tensors (no host
read), the updates are ``addcmul_`` / ``mul_`` + ``add_`` on the strided
interior views (no temporaries), and because the halos of p, q and r are
zero the two inner products are ``torch.dot`` over the flat contiguous
fields.  Those sums are in the field dtype and in torch's order; the
native ones are float64 in a fixed order.

Method: wall time (host clock around a loop that ends in a device
synchronise) of a block of K iterations, divided by K.  Every block starts
from ``start(b, 0)`` outside the timed window, so all contenders do the
same arithmetic on the same data.  The contenders alternate over several
repeats after a warm-up; the median is reported with min and max.  Before
timing, a replayed block is checked bitwise against an eager one, and five
composed iterations against five native ones.

Run on a GPU box:  python benchmarks/bench_stencil_cg.py [--out result.json]
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

W = 1
NU = 100.0  # far from converged within a block, whatever the size
SIZES = {"small": (1, 130, 130), "large": (8, 2050, 4098)}
STREAMS = 11  # field-sized reads + writes of one native iteration


def weights():
    k = torch.zeros(3, 3, dtype=torch.float64)
    k[1, 0] = k[1, 2] = k[0, 1] = k[2, 1] = -NU
    k[1, 1] = 1.0 + 4.0 * NU
    return k


def inner(t):
    return t[..., W:-W, W:-W]


class Composed:
    """The same recurrence from ``apply`` and torch ops (module
    docstring).  No guard for a zero denominator: torch has none."""

    def __init__(self, st, shape, dtype):
        self.st = st
        z = dict(dtype=dtype, device="cuda")
        self.x, self.r = torch.zeros(shape, **z), torch.zeros(shape, **z)
        self.p, self.q = torch.zeros(shape, **z), torch.zeros(shape, **z)
        self.rs = torch.zeros((), **z)

    def start(self, b):
        self.x.zero_()
        inner(self.r).copy_(inner(b))
        inner(self.p).copy_(inner(b))
        self.rs = torch.dot(self.r.view(-1), self.r.view(-1))

    def iterate(self, n):
        x, r, p, q = self.x, self.r, self.p, self.q
        for _ in range(n):
            self.st.apply(p, out=q)
            alpha = self.rs / torch.dot(p.view(-1), q.view(-1))
            inner(x).addcmul_(inner(p), alpha)
            inner(r).addcmul_(inner(q), -alpha)
            rs = torch.dot(r.view(-1), r.view(-1))
            inner(p).mul_(rs / self.rs).add_(inner(r))
            self.rs = rs


class Case:
    def __init__(self, grid, size, dtype, block):
        shape = SIZES[size]
        self.shape, self.dtype, self.block = shape, dtype, block
        self.st = grid.make_stencil(shape, dtype, "cuda", weights())
        torch.manual_seed(0)
        self.b = torch.zeros(shape, dtype=dtype, device="cuda")
        inner(self.b).copy_(torch.randn(
            shape[0], shape[1] - 2 * W, shape[2] - 2 * W, device="cuda"))
        self.cg = self.st.make_cg()
        self.x = torch.zeros_like(self.b)
        self.gcg = self.st.make_cg()
        self.gx = torch.zeros_like(self.b)
        self.composed = Composed(self.st, shape, dtype)
        self.graph = None

    def _restart(self, which):
        if which == "composed":
            self.composed.start(self.b)
        else:
            cg, x = ((self.cg, self.x) if which == "native_eager"
                     else (self.gcg, self.gx))
            x.zero_()
            cg.start(self.b, x)

    def _capture(self):
        self._restart("native_graph")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self.gcg.iterate(self.block)  # warm-up on a side stream
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.gcg.iterate(self.block)

    def run(self, which):
        """One block of ``block`` iterations, enqueued."""
        if which == "native_eager":
            self.cg.iterate(self.block)
        elif which == "native_graph":
            self.graph.replay()
        else:
            self.composed.iterate(self.block)

    def check(self, few=5):
        """The graph replays the eager sequence, so a block of each from
        the same start agrees bitwise.  The composed path rounds
        differently and conjugate gradients amplify that with every
        iteration, so it is compared after ``few`` iterations."""
        self._capture()
        for which in ("native_eager", "native_graph"):
            self._restart(which)
            self.run(which)
        torch.cuda.synchronize()
        assert torch.equal(self.x, self.gx), "graph replay != eager"
        rs_block = self.cg.rs.item()
        self._restart("native_eager")
        self._restart("composed")
        self.cg.iterate(few)
        self.composed.iterate(few)
        ref = inner(self.x).double()
        rel = ((inner(self.composed.x).double() - ref).norm()
               / ref.norm()).item()
        tol = 1e-3 if self.dtype == torch.float32 else 1e-9
        assert rel < tol, f"composed iteration differs by {rel:.2e}"
        return {"composed_vs_native_rel_diff": rel, "after": few,
                "rs_after_block": rs_block}

    def time_block(self, which):
        self._restart(which)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.run(which)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / self.block * 1e6


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--warmup", type=int, default=3,
                   help="untimed blocks per contender")
    p.add_argument("--repeats", type=int, default=9)
    p.add_argument("--block-small", type=int, default=200,
                   help="iterations per timed block of the small size")
    p.add_argument("--block-large", type=int, default=40)
    p.add_argument("--sizes", default="small,large")
    p.add_argument("--out", default=None,
                   help="also write the JSON result to this file")
    args = p.parse_args()

    if not torch.cuda.is_available():
        raise SystemExit("bench_stencil_cg.py measures the GPU path; no "
                         "GPU found")
    m.init()
    grid = CartesianGrid(dims=(1, 1), periodic=(True, True))
    names = ("native_eager", "native_graph", "composed")
    out = {"device": torch.cuda.get_device_name(0),
           "repeats": args.repeats, "unit": "us per iteration"}
    for size in args.sizes.split(","):
        block = args.block_small if size == "small" else args.block_large
        for dtype in (torch.float32, torch.float64):
            case = Case(grid, size, dtype, block)
            res = {"shape": list(SIZES[size]), "block": block,
                   "check": case.check()}
            for which in names:
                for _ in range(args.warmup):
                    case.time_block(which)
            samples = {k: [] for k in names}
            for _ in range(args.repeats):  # alternate the contenders
                for which in names:
                    samples[which].append(case.time_block(which))
            nbytes = STREAMS * case.b.numel() * case.b.element_size()
            for k, s in samples.items():
                med = statistics.median(s)
                res[k] = {"us": round(med, 2),
                          "us_min_max": [round(min(s), 2), round(max(s), 2)],
                          "streams_GBps": round(nbytes / med / 1e3, 1)}
            for k in names[:2]:
                res[f"composed_over_{k}"] = round(
                    res["composed"]["us"] / res[k]["us"], 3)
            out[f"{size}_{str(dtype).split('.')[-1]}"] = res
            del case
            torch.cuda.empty_cache()
    print(json.dumps(out, indent=2))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=2)


if __name__ == "__main__":
    main()
