"""Fourth-order diffusion of a 3-D field with a 2-cell halo.

A user stencil code on top of the reusable halo exchanger
(``CartesianGrid.make_halo_exchanger``): the field is ``(nz, ny, nx)``,
decomposed over a 2-D periodic process grid in (y, x); the leading ``nz``
levels ride along in every message.  The fourth-order Laplacian reaches
two cells out, so the halo is ``width=2``.  One ``exchange_`` per step
refreshes all levels: on the GPU that is one pack launch, one RCCL group
and one unpack launch.

    python examples/wide_stencil_diffusion.py
    python -m mpi4jax_amd.run -n 4 examples/wide_stencil_diffusion.py

The periodic problem conserves the field's total, which is checked at the
end across all ranks.
"""

import argparse
import time

import torch

import os as _os, sys as _sys
_sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))

import mpi4jax_amd as m
from mpi4jax_amd.parallel import CartesianGrid

W = 2  # halo width of the fourth-order stencil


def laplacian4(u):
    """Fourth-order 5+5-point Laplacian of the interior of ``u``."""
    c = u[:, W:-W, W:-W]
    d2x = (-u[:, W:-W, :-4] + 16.0 * u[:, W:-W, 1:-3] - 30.0 * c
           + 16.0 * u[:, W:-W, 3:-1] - u[:, W:-W, 4:]) / 12.0
    d2y = (-u[:, :-4, W:-W] + 16.0 * u[:, 1:-3, W:-W] - 30.0 * c
           + 16.0 * u[:, 3:-1, W:-W] - u[:, 4:, W:-W]) / 12.0
    return d2x + d2y


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--size", type=int, default=128,
                   help="global interior cells per horizontal axis")
    p.add_argument("--nz", type=int, default=4)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--device", default=None)
    args = p.parse_args()

    m.init()
    comm = m.get_world()
    device = args.device or ("cuda" if torch.cuda.is_available() else "cpu")
    grid = CartesianGrid(comm=comm, periodic=(True, True))
    if args.size % grid.nproc_y or args.size % grid.nproc_x:
        raise SystemExit(f"--size {args.size} must divide over the process grid "
                         f"{grid.nproc_y}x{grid.nproc_x}")
    by, bx = args.size // grid.nproc_y, args.size // grid.nproc_x
    cy, cx = grid.coords

    # a Gaussian bump per level, centred in the global domain
    y = (torch.arange(by, dtype=torch.float64) + cy * by + 0.5) / args.size
    x = (torch.arange(bx, dtype=torch.float64) + cx * bx + 0.5) / args.size
    z = torch.arange(1, args.nz + 1, dtype=torch.float64)
    bump = torch.exp(-((y[:, None] - 0.5) ** 2 + (x[None, :] - 0.5) ** 2)
                     / 0.01)
    u = torch.zeros(args.nz, by + 2 * W, bx + 2 * W, dtype=torch.float64,
                    device=device)
    u[:, W:-W, W:-W] = (z[:, None, None] * bump).to(device)

    ex = grid.make_halo_exchanger(u.shape, u.dtype, device, width=W)
    total0 = m.allreduce(u[:, W:-W, W:-W].sum(), m.SUM, comm=comm).item()

    t0 = time.perf_counter()
    for _ in range(args.steps):
        ex.exchange_(u)
        u[:, W:-W, W:-W] += 0.1 * laplacian4(u)
    if device == "cuda":
        torch.cuda.synchronize()
    wall = time.perf_counter() - t0

    total = m.allreduce(u[:, W:-W, W:-W].sum(), m.SUM, comm=comm).item()
    peak = m.allreduce(u[:, W:-W, W:-W].max(), m.MAX, comm=comm).item()
    drift = abs(total - total0) / abs(total0)
    assert drift < 1e-12, f"total drifted by {drift:.2e}"
    assert peak < float(args.nz), "diffusion must lower the peak"
    if comm.rank == 0:
        print(f"n={args.size} nz={args.nz} device={device}: peak {peak:.6f}, "
              f"total drift {drift:.1e}, {wall:.3f}s")
        print(f"OK: {args.steps} steps over {comm.size} rank(s)")


if __name__ == "__main__":
    main()
