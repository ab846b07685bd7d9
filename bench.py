"""Flagship benchmark: shallow-water steps/sec + the BASELINE comm configs.

Measures the reference's headline benchmark (BASELINE.json / BASELINE.md):
the shallow-water demo on a (3600, 1800) float32 domain
(``/root/reference/docs/shallow-water.rst:49-52``), reported as whole-job
steps/sec (strong scaling: fixed global domain decomposed over N GPUs),
plus every communication config BASELINE.json names, each labeled with
n_gpus so the driver's multi-GPU run produces the complete headline:

* config #2 — 256 MiB bf16 allreduce, enqueued inside a captured hipGraph
  (the "in-jit" analog; falls back to eager enqueue with ``in_graph:
  false`` if capture fails on the box).  At n_gpus=1 this is a local
  device copy, NOT communication — labeled as such.
* config #4 — alltoall + allgather at 1 GiB/rank (xGMI bisection).
* config #5 — torch.autograd backward through allreduce(SUM) bf16.

Launch (driver contract):
    python bench.py --gpus N --steps K --warmup W
N>1 runs under torch.distributed.run with one rank per GPU over RCCL.
Such a plain run measures only the shallow-water headline: K timed steps
after W warm-up steps, one JSON line.  ``--full`` adds the communication
configs above to that line; ``--dump-outputs DIR`` writes the state of
the last timed step as ``DIR/<name>.npy``.

``--preflight`` instead validates the N>1 machinery end-to-end over the
gloo bootstrap plane (CPU): decomposed model steps, cross-rank halo
schedule matching, the stepper's all-or-none graph-adoption agreement —
so the first multi-GPU contact cannot die on schedule bugs.

vs_baseline compares seconds-per-model-day against the reference's
published GPU n=1 number (103.18 s/model-day on a Tesla P100,
docs/shallow-water.rst:81-83).
"""

import argparse
import json
import os
import time

import torch

import mpi4jax_amd as m
from mpi4jax_amd.models import ShallowWater
from mpi4jax_amd.parallel.grid import default_dims

REF_SEC_PER_MODEL_DAY_GPU1 = 103.18  # P100, docs/shallow-water.rst:81-83


def _timed_region(fn, steps, comm):
    """barrier+sync bracketed timing; returns max-over-ranks seconds/step."""
    m.barrier(comm=comm)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    m.barrier(comm=comm)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    dt_t = torch.tensor([dt], dtype=torch.float64)
    return m.allreduce(dt_t, m.MAX, comm=comm).item()


def bench_allreduce_graph(comm, nbytes=256 * 1024 * 1024, iters=20,
                          warmup=5):
    """BASELINE config #2: 256 MiB bf16 allreduce inside a hipGraph."""
    n = nbytes // 2
    x = torch.randn(n, device="cuda").to(torch.bfloat16)
    m.allreduce(x, m.SUM, comm=comm)  # comm init + warm path
    try:  # register the persistent buffer for RCCL zero-copy protocols
        from mpi4jax_amd._backend import rccl

        rccl.ext().comm_register(comm.rccl_handle(), x)
    except Exception:
        pass
    for _ in range(warmup):
        m.allreduce(x, m.SUM, comm=comm)
    torch.cuda.synchronize()

    in_graph = True
    per_replay = 4
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(per_replay):
                m.allreduce(x, m.SUM, comm=comm)
        g.replay()
        torch.cuda.synchronize()
        step = g.replay
    except Exception:
        in_graph = False
        per_replay = 1
        torch.cuda.synchronize()

        def step():
            m.allreduce(x, m.SUM, comm=comm)

    dt = _timed_region(step, iters, comm) / per_replay
    size = comm.size
    algbw = nbytes / dt / 1e9
    busbw = algbw * (2 * (size - 1) / size) if size > 1 else algbw
    out = {"algbw_GBps": round(algbw, 2), "busbw_GBps": round(busbw, 2),
           "bytes": nbytes, "dtype": "bf16", "in_graph": in_graph,
           "n_gpus": size}
    if size == 1:
        out["note"] = "single rank: local device copy, NOT communication"
    return out


def bench_alltoall_allgather(comm, per_rank_bytes=1 << 30, iters=10,
                             warmup=3):
    """BASELINE config #4: alltoall + allgather, 1 GiB/rank, bf16."""
    size = comm.size
    res = {}

    n = per_rank_bytes // 2 // size * size  # divisible by nproc
    x = torch.randn(n, device="cuda").to(torch.bfloat16).reshape(size, -1)
    m.alltoall(x, comm=comm)
    for _ in range(warmup):
        m.alltoall(x, comm=comm)
    dt = _timed_region(lambda: m.alltoall(x, comm=comm), iters, comm)
    nbytes = n * 2
    algbw = nbytes / dt / 1e9
    res["alltoall"] = {
        "algbw_GBps": round(algbw, 2),
        "busbw_GBps": round(algbw * (size - 1) / size, 2),
        "bytes_per_rank": nbytes, "dtype": "bf16", "n_gpus": size,
    }
    del x

    ng = per_rank_bytes // 2 // size  # input so the gathered output is 1 GiB
    y = torch.randn(ng, device="cuda").to(torch.bfloat16)
    m.allgather(y, comm=comm)
    for _ in range(warmup):
        m.allgather(y, comm=comm)
    dt = _timed_region(lambda: m.allgather(y, comm=comm), iters, comm)
    out_bytes = ng * 2 * size
    algbw = out_bytes / dt / 1e9
    res["allgather"] = {
        "algbw_GBps": round(algbw, 2),
        "busbw_GBps": round(algbw * (size - 1) / size, 2),
        "bytes_gathered": out_bytes, "dtype": "bf16", "n_gpus": size,
    }
    if size == 1:
        for v in res.values():
            v["note"] = "single rank: local device copy, NOT communication"
    return res


def bench_grad_allreduce(comm, nbytes=256 * 1024 * 1024, iters=10,
                         warmup=3):
    """BASELINE config #5: torch.autograd backward through allreduce(SUM).

    The VJP of allreduce-SUM is the identity (reference
    allreduce.py:152-159), so the measured region is forward comm +
    autograd machinery — the reference's ``jax.grad`` config."""
    n = nbytes // 2
    w = torch.randn(n, device="cuda", dtype=torch.bfloat16,
                    requires_grad=True)

    def step():
        y = m.allreduce(w, m.SUM, comm=comm)
        y.float().sum().backward()
        w.grad = None

    step()
    for _ in range(warmup):
        step()
    dt = _timed_region(step, iters, comm)
    size = comm.size
    algbw = nbytes / dt / 1e9
    return {"ms": round(dt * 1e3, 3), "fwd_algbw_GBps": round(algbw, 2),
            "bytes": nbytes, "dtype": "bf16", "n_gpus": size,
            "note": "VJP of allreduce(SUM) is the identity; timed region "
                    "= forward comm + full autograd pass"}


def preflight():
    """Validate the N>1 machinery over gloo (CPU) — exits nonzero on any
    failure.  Covers: decomposed model stepping, cross-rank halo schedule
    send/recv matching, flat-schedule encoding, and the all-or-none
    graph-adoption agreement reduction."""
    import sys

    from mpi4jax_amd.parallel.grid import (CartesianGrid,
                                           halo_exchange_schedule)

    m.init()
    comm = m.get_world()
    n = comm.size
    dims = default_dims(n)
    failures = []

    # 1. decomposed model steps and stays finite
    sw = ShallowWater(nx=360, ny=180, comm=comm, dims=dims, device="cpu",
                      dtype=torch.float64)
    state = sw.initial_conditions()
    state = sw.step(state, first_step=True)
    for _ in range(10):
        state = sw.step(state)
    if not torch.isfinite(state.h).all():
        failures.append("model diverged at world %d" % n)

    # 2. halo schedule cross-rank matching: every rank's sends to peer p
    # must pair with p's recvs from this rank, in count and size
    grid = CartesianGrid(comm=comm, dims=dims)
    ny, nx = sw.ny_local, sw.nx_local
    _, col_ops, row_ops, cor_ops, _ = halo_exchange_schedule(grid, nx, ny)
    sends, recvs = [], []
    for k, st, rf, sidx, ridx in col_ops:
        if st is not None:
            sends.append((st, "col", ny))
        if rf is not None:
            recvs.append((rf, "col", ny))
    for st, rf, ridx, sidx in row_ops:
        if st is not None:
            sends.append((st, "row", nx - 2))
        if rf is not None:
            recvs.append((rf, "row", nx - 2))
    for d, st, rf in cor_ops:
        if st is not None:
            sends.append((st, "cor", 1))
        if rf is not None:
            recvs.append((rf, "cor", 1))
    all_sends = comm._allgather_py(sends)
    all_recvs = comm._allgather_py(recvs)
    for r in range(n):
        for p in range(n):
            s = [(kind, sz) for (to, kind, sz) in all_sends[r] if to == p]
            q = [(kind, sz) for (frm, kind, sz) in all_recvs[p] if frm == r]
            if s != q:
                failures.append(
                    f"schedule mismatch {r}->{p}: sends {s} != recvs {q}")

    # 3. stepper path (eager on CPU) + agreement reduction semantics
    advance, state = sw.make_stepper(state, steps_per_call=2)
    state = advance()
    if not torch.isfinite(state.h).all():
        failures.append("stepper diverged")
    if sw._all_ranks_agree(True) is not True:
        failures.append("agree(True) != True")
    if sw._all_ranks_agree(comm.rank != 0) is not False:
        failures.append("agree(mixed) != False")

    all_fail = [x for fl in comm._allgather_py(failures) for x in fl]
    if comm.rank == 0:
        if all_fail:
            print("PREFLIGHT_FAILED:", all_fail, flush=True)
        else:
            print(f"PREFLIGHT_OK world_size={n} dims={dims}", flush=True)
    sys.exit(1 if all_fail else 0)


DUMP_BUDGET_BYTES = 60 * 1000 * 1000  # keeps the files under 64 MB in all
DUMP_SAMPLE_SEED = 20240531


def dump_outputs(sw, state, outdir):
    """Write the model state the timed path returned from its last step
    (h, u, v and the AB2 tendencies dh, du, dv) as ``outdir/<name>.npy``.

    At world size 1 these are the local arrays, halo ring included; at
    N>1 each field's interior is gathered onto rank 0, which writes it.
    Arrays keep the model dtype (float32 here).  If the fields together
    exceed the budget, every field is reduced to the same fixed, seeded
    sample of its flattened elements (indices ascending), so two builds
    run with the same arguments write comparable files."""
    import numpy as np

    fields = {}
    for name in state._fields:
        f = getattr(state, name)
        if sw.comm.size > 1:
            f = sw.gather_global(f)  # collective: every rank takes part
        if f is not None:
            fields[name] = f.detach().to("cpu").contiguous().numpy()
    if sw.comm.rank != 0:
        return
    total = sum(a.nbytes for a in fields.values())
    if total > DUMP_BUDGET_BYTES:
        numel = next(iter(fields.values())).size
        itemsize = max(a.itemsize for a in fields.values())
        keep = DUMP_BUDGET_BYTES // (len(fields) * itemsize)
        rng = np.random.default_rng(DUMP_SAMPLE_SEED)
        idx = np.sort(rng.choice(numel, size=min(keep, numel),
                                 replace=False))
        fields = {k: a.reshape(-1)[idx] for k, a in fields.items()}
    os.makedirs(outdir, exist_ok=True)
    for name, a in fields.items():
        np.save(os.path.join(outdir, name + ".npy"), a)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=1000)
    p.add_argument("--warmup", type=int, default=100)
    p.add_argument("--nx", type=int, default=3600)
    p.add_argument("--ny", type=int, default=1800)
    p.add_argument("--preflight", action="store_true")
    p.add_argument("--full", action="store_true",
                   help="after the shallow-water metric, also measure the "
                        "BASELINE communication configs (off by default)")
    p.add_argument("--skip-comm-bench", action="store_true",
                   help="only the shallow-water metric, even with --full")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="write the last timed step's state as DIR/<name>.npy")
    args = p.parse_args()
    if args.steps < 1:
        p.error("--steps must be at least 1")

    if args.preflight:
        preflight()
        return

    m.init()
    comm = m.get_world()
    rank = comm.rank
    n = comm.size
    use_gpu = torch.cuda.is_available()
    device = "cuda" if use_gpu else "cpu"

    dims = default_dims(n)
    sw = ShallowWater(nx=args.nx, ny=args.ny, comm=comm, dims=dims,
                      device=device, dtype=torch.float32)
    try:
        state = sw.initial_conditions()
        state = sw.step(state, first_step=True)
        state = sw.step(state)
    except Exception as e:  # robustness: fall back to the eager op path
        if not sw.fused:
            raise
        print(f"# fused path failed ({e!r}); falling back to eager",
              flush=True)
        sw = ShallowWater(nx=args.nx, ny=args.ny, comm=comm, dims=dims,
                          device=device, dtype=torch.float32, fused=False)
        state = sw.initial_conditions()
        state = sw.step(state, first_step=True)

    # warmup (untimed) + hipGraph capture of a multistep
    for _ in range(args.warmup):
        state = sw.step(state)

    # all-rank finiteness gate after warmup: if the fused step ever
    # misbehaves on a topology this pool could not test (ROADMAP #1),
    # fall back LOUDLY to the two-kernel pipeline rather than dying —
    # the fallback is printed and carried in the result JSON.
    fused_fallback = False
    if sw.fused:
        ok = torch.isfinite(state.h).all().to(torch.float32).cpu()
        ok = m.allreduce(ok, m.MIN, comm=comm).item()
        if ok < 1.0:
            import os as _os

            print("# fused step went non-finite after warmup; "
                  "falling back to MPI4JAX_AMD_SW_NOFUSE=1", flush=True)
            _os.environ["MPI4JAX_AMD_SW_NOFUSE"] = "1"
            fused_fallback = True
            sw = ShallowWater(nx=args.nx, ny=args.ny, comm=comm,
                              dims=dims, device=device,
                              dtype=torch.float32)
            state = sw.step(sw.initial_conditions(), first_step=True)
            for _ in range(args.warmup):
                state = sw.step(state)
    # steps per captured graph: bigger graphs amortize replay-launch
    # overhead (87k-step soak measures 0.0911 ms/step at spc=500 vs
    # 0.101 at spc=10); capture+validation cost stays untimed either way
    if args.steps >= 250:
        spc = 50
    elif args.steps > 50:
        spc = 10
    else:
        # graph capture needs an even step count (buffer parity); an odd
        # --steps runs its last step through the plain step below
        spc = args.steps - args.steps % 2
    if spc:
        advance, state = sw.make_stepper(state, steps_per_call=spc)
        advance()  # one warm replay
        n_calls, rem = divmod(args.steps, spc)
    else:
        n_calls, rem = 0, args.steps

    m.barrier()
    if use_gpu:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n_calls):
        state = advance()
    for _ in range(rem):
        state = sw.step(state)
    m.barrier()
    if use_gpu:
        torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0

    # MAX over ranks (job time = slowest rank)
    elapsed_t = torch.tensor([elapsed], dtype=torch.float64)
    elapsed = m.allreduce(elapsed_t, m.MAX, comm=comm).item()

    # sanity: the state must still be finite (no skipped work)
    assert torch.isfinite(state.h).all(), "model diverged"

    steps_per_sec = args.steps / elapsed
    ms_per_step = elapsed / args.steps * 1000
    spd = sw.steps_per_model_day()
    sec_per_model_day = spd / steps_per_sec

    if args.dump_outputs:
        dump_outputs(sw, state, args.dump_outputs)

    comm_bench = {}
    if args.full and use_gpu and not args.skip_comm_bench:
        for name, fn in (
            ("allreduce_256MiB_bf16", lambda: bench_allreduce_graph(comm)),
            ("bisection_1GiB_bf16",
             lambda: bench_alltoall_allgather(comm)),
            ("grad_allreduce_256MiB_bf16",
             lambda: bench_grad_allreduce(comm)),
        ):
            try:
                comm_bench[name] = fn()
            except Exception as e:
                comm_bench[name] = {"error": repr(e)}

    if rank == 0:
        result = {
            "metric": "shallow_water_steps_per_sec",
            "value": round(steps_per_sec, 3),
            "unit": "steps/s",
            "n_gpus": n,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": round(REF_SEC_PER_MODEL_DAY_GPU1
                                 / sec_per_model_day, 3),
            "dtype": "fp32",
            "data": "synthetic",
            "config": {
                "model": "shallow_water",
                "domain": [args.ny, args.nx],
                "sec_per_model_day": round(sec_per_model_day, 2),
                "parallelism": f"domain-decomposition {dims[0]}x{dims[1]}",
                "fused_kernels": sw.fused,
                "fused_fallback": fused_fallback,
                **comm_bench,
            },
        }
        print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
