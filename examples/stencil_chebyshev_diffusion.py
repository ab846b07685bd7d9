"""Implicit diffusion: Chebyshev iteration over the fused halo stencil.

Backward Euler for ``u_t = lap(u)`` on a periodic, decomposed grid: every
step solves ``(I - nu * lap) u_new = u`` with ``nu = dt / dx^2`` above the
explicit limit of 1/4, as examples/stencil_cg_diffusion.py does with
conjugate gradients.  Here the solver is ``HaloStencil.make_chebyshev``
with the bounds ``HaloStencil.gershgorin_bounds()`` gives for free,
``(1, 1 + 8 nu)`` for this operator: one launch per iteration, no inner
product and, across ranks, no collective besides the halo exchange.  The
number of iterations is known before the first one
(``iterations_for(rtol)``), so ``solve(..., check_every=0)`` runs them
without ever reading a residual back.  The previous step is the first
guess of the next.

    python examples/stencil_chebyshev_diffusion.py
    python -m mpi4jax_amd.run -n 2 examples/stencil_chebyshev_diffusion.py

The iteration count grows like ``sqrt(1 + 8 nu)`` and conjugate gradients
need fewer iterations; Chebyshev wins where an iteration is cheap enough
and an allreduce dear enough (docs/usage.md).  The periodic problem
conserves the field's total, and the true residual
``||u - A u_new|| / ||u||`` of every step is recomputed with ``apply``;
both are checked across all ranks.
"""

import argparse
import math
import time

import torch

import os as _os, sys as _sys
_sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))

import mpi4jax_amd as m
from mpi4jax_amd.parallel import CartesianGrid

W = 1  # halo width of the 5-point stencil


def implicit_weights(nu):
    """``I - nu * lap`` as a 3x3 table; entry [a][b] multiplies the cell
    at offset (a - 1, b - 1)."""
    k = torch.zeros(3, 3, dtype=torch.float64)
    k[1, 0] = k[1, 2] = k[0, 1] = k[2, 1] = -nu
    k[1, 1] = 1.0 + 4.0 * nu
    return k


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--size", type=int, default=128,
                   help="global interior cells per horizontal axis")
    p.add_argument("--nz", type=int, default=4)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--nu", type=float, default=4.0)
    p.add_argument("--rtol", type=float, default=1e-10)
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
    y = (torch.arange(by, dtype=torch.float64) + cy * by + 0.5) / args.size
    x = (torch.arange(bx, dtype=torch.float64) + cx * bx + 0.5) / args.size
    z = torch.arange(1, args.nz + 1, dtype=torch.float64)[:, None, None]

    shape = (args.nz, by + 2 * W, bx + 2 * W)
    st = grid.make_stencil(shape, torch.float64, device,
                           implicit_weights(args.nu))
    lmin, lmax = st.gershgorin_bounds()  # (1, 1 + 8 nu)
    cheb = st.make_chebyshev(lmin, lmax)
    per_step = cheb.iterations_for(args.rtol)

    u = torch.zeros(shape, dtype=torch.float64, device=device)
    bump = torch.exp(-((y[:, None] - 0.5) ** 2 + (x[None, :] - 0.5) ** 2)
                     / 0.01)
    u[:, W:-W, W:-W] = (z * bump).to(device)
    check = torch.zeros_like(u)

    def total(f):
        return m.allreduce(f[:, W:-W, W:-W].sum(), m.SUM, comm=comm).item()

    total0 = total(u)
    iterations, worst = 0, 0.0
    t0 = time.perf_counter()
    for _ in range(args.steps):
        # the a-priori count: nothing is reduced, nothing read back
        new, info = cheb.solve(u, u, rtol=args.rtol, check_every=0)
        iterations += info.iterations
        # the true residual, not the recurrence's (the example's own check)
        st.apply(new, out=check)
        res = check.sub_(u)
        worst = max(worst, math.sqrt(st.dot(res, res).item()
                                     / st.dot(u, u).item()))
        u = new
    if device == "cuda":
        torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    peak = m.allreduce(u[:, W:-W, W:-W].max(), m.MAX, comm=comm).item()
    drift = abs(total(u) - total0) / abs(total0)
    assert drift < 1e-9, f"total drifted by {drift:.2e}"
    assert worst < 10 * args.rtol, f"true residual {worst:.2e}"
    assert peak < float(args.nz), "diffusion must lower the peak"

    if comm.rank == 0:
        print(f"n={args.size} nz={args.nz} device={device} nu={args.nu}: "
              f"bounds ({lmin:g}, {lmax:g}), {per_step} iterations per step, "
              f"peak {peak:.6f}, total drift {drift:.1e}, worst true "
              f"residual {worst:.1e}, {iterations} Chebyshev iterations, "
              f"{wall:.3f}s")
        print(f"OK: {args.steps} implicit steps over {comm.size} rank(s)")


if __name__ == "__main__":
    main()
