"""Heterogeneous diffusion: CG over the variable-coefficient halo stencil.

Solves ``(I - div(k grad)) u = b`` on a periodic, decomposed grid with a
conductivity ``k(y, x)`` that varies by a factor of 100.  The operator is
one ``CartesianGrid.make_variable_stencil``: five taps, one coefficient
plane each.  ``k`` is built locally and exchanged once so that its halo
holds the neighbours' values; a face coefficient is minus the mean of the
two cells it separates, which makes the assembled operator symmetric
across rank edges too, and the centre is 1 minus the four faces.
``make_cg().solve`` then runs as for the constant stencil.

    python examples/variable_diffusion_cg.py
    python -m mpi4jax_amd.run -n 2 examples/variable_diffusion_cg.py
"""

import argparse
import math

import torch

import os as _os, sys as _sys
_sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))

import mpi4jax_amd as m
from mpi4jax_amd.parallel import CartesianGrid

OFFSETS = [(0, 0), (-1, 0), (0, -1), (0, 1), (1, 0)]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--size", type=int, default=128,
                   help="global interior cells per horizontal axis")
    p.add_argument("--nz", type=int, default=4)
    p.add_argument("--rtol", type=float, default=1e-10)
    p.add_argument("--device", default=None)
    args = p.parse_args()

    m.init()
    comm = m.get_world()
    device = args.device or ("cuda" if torch.cuda.is_available() else "cpu")
    grid = CartesianGrid(comm=comm, periodic=(True, True))
    if args.size % grid.nproc_y or args.size % grid.nproc_x:
        raise SystemExit(f"--size {args.size} must divide over the process "
                         f"grid {grid.nproc_y}x{grid.nproc_x}")
    by, bx = args.size // grid.nproc_y, args.size // grid.nproc_x
    cy, cx = grid.coords
    y = (torch.arange(by, dtype=torch.float64) + cy * by + 0.5) / args.size
    x = (torch.arange(bx, dtype=torch.float64) + cx * bx + 0.5) / args.size
    ny, nx = by + 2, bx + 2
    shape = (args.nz, ny, nx)

    # conductivity in [0.1, 10], its halo filled from the neighbours
    k = torch.zeros(ny, nx, dtype=torch.float64, device=device)
    k[1:-1, 1:-1] = (10.0 ** (torch.sin(2 * math.pi * y)[:, None]
                              * torch.cos(4 * math.pi * x)[None, :])).to(device)
    k = grid.make_halo_exchanger(k.shape, k.dtype, device).exchange(k)
    coef = torch.zeros(5, ny, nx, dtype=torch.float64, device=device)
    for t, (dy, dx) in enumerate(OFFSETS[1:], 1):
        coef[t, 1:-1, 1:-1] = -0.5 * (
            k[1:-1, 1:-1] + k[1 + dy:ny - 1 + dy, 1 + dx:nx - 1 + dx])
    coef[0] = 1.0 - coef[1:].sum(0)

    st = grid.make_variable_stencil(shape, torch.float64, device, OFFSETS,
                                    coef)
    b = torch.zeros(shape, dtype=torch.float64, device=device)
    z = torch.arange(1, args.nz + 1, dtype=torch.float64)[:, None, None]
    b[:, 1:-1, 1:-1] = (z * torch.exp(
        -((y[:, None] - 0.5) ** 2 + (x[None, :] - 0.5) ** 2) / 0.01)
    ).to(device)

    u, info = st.make_cg().solve(b, rtol=args.rtol, maxiter=2000)
    assert info.converged, f"no convergence in {info.iterations}"
    res = st.apply(u).sub_(b)  # the true residual, not the recurrence's
    true = math.sqrt(st.dot(res, res).item()) / info.rhs_norm
    assert true < 10 * args.rtol, f"true residual {true:.2e}"
    # every row of A sums to 1 on a periodic grid: the total is conserved
    tot = [m.allreduce(f[:, 1:-1, 1:-1].sum(), m.SUM, comm=comm).item()
           for f in (u, b)]
    assert abs(tot[0] - tot[1]) < 1e-8 * abs(tot[1]), tot
    if comm.rank == 0:
        print(f"n={args.size} nz={args.nz} device={device}: "
              f"{info.iterations} CG iterations, true residual {true:.1e}")
        print(f"OK: variable diffusion solved over {comm.size} rank(s)")


if __name__ == "__main__":
    main()
