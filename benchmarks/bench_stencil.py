"""Fused halo stencil timing at world 1 (periodic in both axes).

Workloads: ``w2`` is one float32 field (8, 1806, 3606) at width 2 with the
fourth-order diffusion star (identity + 0.1 * Laplacian, 9 taps); ``w1`` is
three float32 fields (1802, 3602) at width 1 with the second-order star
(5 taps).

(a) ``apply(u, out=v)`` against the slicing path the library offered
    before: ``exchange_`` followed by the in-place slicing update of
    ``examples/wide_stencil_diffusion.py``;
(b) ``apply(u, out=v)`` against ``v.copy_(u)`` on the same tensors: the
    copy moves the same bytes once and is the traffic floor;
(c) ``w2`` only: forward and backward through K = 8 steps of ``apply_ad``
    against the same through ``exchange_ad`` plus slicing, with the peak
    of ``torch.cuda.max_memory_allocated``.

Per contender: wall time per call (host clock around a loop that ends in a
device synchronise).  The contenders of a case alternate over several
repeats; the median is reported next to min/max so the spread is visible.
Before timing, the fused result is checked against a float64 evaluation
of the same taps within the a-priori bound gamma(n + 2) * sum|K||x|, and
the slicing path within that plus gamma(16) * sum|K||x| for its own, longer
chain of roundings.

Run on a GPU box:  python benchmarks/bench_stencil.py [--out result.json]
``--profile N`` runs only N fused applies of ``w2`` after a warm-up — the
body of a ``rocprofv3 --kernel-trace --stats`` run.
"""

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import mpi4jax_amd as m  # noqa: E402
from mpi4jax_amd.parallel import CartesianGrid  # noqa: E402

NU = 0.1


def lap4(u, W=2):
    c = u[..., W:-W, W:-W]
    d2x = (-u[..., W:-W, :-4] + 16.0 * u[..., W:-W, 1:-3] - 30.0 * c
           + 16.0 * u[..., W:-W, 3:-1] - u[..., W:-W, 4:]) / 12.0
    d2y = (-u[..., :-4, W:-W] + 16.0 * u[..., 1:-3, W:-W] - 30.0 * c
           + 16.0 * u[..., 3:-1, W:-W] - u[..., 4:, W:-W]) / 12.0
    return d2x + d2y


def lap2(u):
    c = u[..., 1:-1, 1:-1]
    return (u[..., 1:-1, :-2] + u[..., 1:-1, 2:] + u[..., :-2, 1:-1]
            + u[..., 2:, 1:-1] - 4.0 * c)


def weights(width):
    n = 2 * width + 1
    k = torch.zeros(n, n, dtype=torch.float64)
    axis = (torch.tensor([-1.0, 16.0, -30.0, 16.0, -1.0]) / 12.0
            if width == 2 else torch.tensor([1.0, -2.0, 1.0])).double()
    k[width, :] += NU * axis
    k[:, width] += NU * axis
    k[width, width] += 1.0
    return k


WORKLOADS = {"w2": ((8, 1806, 3606), 2, 1), "w1": ((1802, 3602), 1, 3)}


def _gamma(k, u=2.0 ** -24):
    return k * u / (1.0 - k * u)


class Workload:
    def __init__(self, grid, name):
        shape, w, nf = WORKLOADS[name]
        self.w, self.nf, self.shape = w, nf, shape
        self.lap = lap4 if w == 2 else lap2
        self.k = weights(w)
        torch.manual_seed(0)
        self.u = [torch.randn(shape, device="cuda") for _ in range(nf)]
        self.v = [torch.zeros(shape, device="cuda") for _ in range(nf)]
        self.s = [t.clone() for t in self.u]  # the slicing path's fields
        self.st = grid.make_stencil(shape, torch.float32, "cuda", self.k,
                                    nfields=nf)
        self.ex = self.st.exchanger

    def fused(self):
        self.st.apply(*self.u, out=self.v)

    def slicing(self):
        w = self.w
        self.ex.exchange_(*self.s)
        for f in self.s:
            f[..., w:-w, w:-w] += NU * self.lap(f)

    def copy(self):
        for a, b in zip(self.v, self.u):
            a.copy_(b)

    def check(self):
        """Both contenders against float64 on the first field."""
        w, n = self.w, int((self.k != 0).sum())
        ny, nx = self.shape[-2:]
        e = self.ex.exchange(*self.u)
        e = (e if isinstance(e, torch.Tensor) else e[0]).double()
        exact = torch.zeros_like(e[..., w:-w, w:-w])
        mag = torch.zeros_like(exact)
        for a in range(2 * w + 1):
            for b in range(2 * w + 1):
                c = self.k[a, b].item()
                if c:
                    t = e[..., a:ny - 2 * w + a, b:nx - 2 * w + b]
                    exact += c * t
                    mag += abs(c) * t.abs()
        del e
        self.fused()
        self.slicing()
        inner = (Ellipsis, slice(w, -w), slice(w, -w))
        err_f = (self.v[0][inner].double() - exact).abs()
        err_s = (self.s[0][inner].double() - exact).abs()
        ok_f = bool((err_f <= _gamma(n + 2) * mag).all())
        ok_s = bool((err_s <= (_gamma(n + 2) + _gamma(16)) * mag).all())
        assert ok_f, f"fused path off by {err_f.max().item():.3e}"
        assert ok_s, f"slicing path off by {err_s.max().item():.3e}"
        return {"fused_max_err": err_f.max().item(),
                "slicing_max_err": err_s.max().item()}


def _time(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def _compare(contenders, warmup, iters, repeats, memory=False):
    for fn in contenders.values():
        for _ in range(warmup):
            fn()
    samples = {k: [] for k in contenders}
    peak = {k: 0 for k in contenders}
    for _ in range(repeats):  # alternate the contenders
        for k, fn in contenders.items():
            if memory:
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
            samples[k].append(_time(fn, iters))
            if memory:
                peak[k] = max(peak[k], torch.cuda.max_memory_allocated())
    out = {}
    for k, s in samples.items():
        out[k] = {"wall_us": round(statistics.median(s), 2),
                  "wall_us_min_max": [round(min(s), 2), round(max(s), 2)]}
        if memory:
            out[k]["max_memory_allocated_MiB"] = round(peak[k] / 2 ** 20, 1)
    return out


def _ratio(res, num, den):
    res[f"{num}_over_{den}"] = round(
        res[num]["wall_us"] / res[den]["wall_us"], 3)
    lo, hi = res[num]["wall_us_min_max"], res[den]["wall_us_min_max"]
    res["ranges_overlap"] = not (lo[1] < hi[0] or hi[1] < lo[0])
    return res


def backward_contenders(wl, steps):
    """Forward + backward through ``steps`` steps, from the interior."""
    w = wl.w
    pad = (w, w, w, w)
    torch.manual_seed(3)
    x0 = torch.randn(wl.shape[:-2] + (wl.shape[-2] - 2 * w,
                                      wl.shape[-1] - 2 * w),
                     device="cuda", requires_grad=True)

    def fused():
        x0.grad = None
        u = F.pad(x0, pad)
        for _ in range(steps):
            u = wl.st.apply_ad(u)
        u[..., w:-w, w:-w].square().sum().backward()

    def slicing():
        x0.grad = None
        inner = x0
        for _ in range(steps):
            u = wl.ex.exchange_ad(F.pad(inner, pad))
            inner = u[..., w:-w, w:-w] + NU * wl.lap(u)
        inner.square().sum().backward()

    # the two gradients agree to float32 rounding first
    fused()
    g1 = x0.grad.clone()
    slicing()
    rel = ((x0.grad - g1).norm() / g1.norm()).item()
    assert rel < 1e-5, rel
    return {"apply_ad": fused, "exchange_ad_slicing": slicing}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--steps", type=int, default=8,
                   help="K of case (c)")
    p.add_argument("--profile", type=int, default=0)
    p.add_argument("--cases", default="abc")
    p.add_argument("--out", default=None,
                   help="also write the JSON result to this file")
    args = p.parse_args()

    if not torch.cuda.is_available():
        raise SystemExit("bench_stencil.py measures the GPU path; no GPU "
                         "found")
    m.init()
    grid = CartesianGrid(dims=(1, 1), periodic=(True, True))

    if args.profile:
        wl = Workload(grid, "w2")
        wl.fused()  # warm-up: loads the code object
        torch.cuda.synchronize()
        for _ in range(args.profile):
            wl.fused()
        torch.cuda.synchronize()
        print(f"profiled {args.profile} fused applies of w2")
        return

    out = {"device": torch.cuda.get_device_name(0), "iters": args.iters,
           "repeats": args.repeats}
    run = (args.warmup, args.iters, args.repeats)
    for name in WORKLOADS:
        wl = Workload(grid, name)
        res = {"check": wl.check()}
        if "a" in args.cases:
            res["a"] = _ratio(_compare(
                {"fused": wl.fused, "slicing": wl.slicing}, *run),
                "slicing", "fused")
        if "b" in args.cases:
            res["b"] = _ratio(_compare(
                {"fused": wl.fused, "copy": wl.copy}, *run),
                "fused", "copy")
        if "c" in args.cases and name == "w2":
            res["c"] = _ratio(_compare(
                backward_contenders(wl, args.steps), 2,
                max(1, args.iters // 20), args.repeats, memory=True),
                "exchange_ad_slicing", "apply_ad")
            res["c"]["steps"] = args.steps
        out[name] = res
        del wl
        torch.cuda.empty_cache()
    print(json.dumps(out, indent=2))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=2)


if __name__ == "__main__":
    main()
