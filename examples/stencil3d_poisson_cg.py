"""3-D Helmholtz solve: CG over the 3-D halo stencil.

Solves ``(I - nu * lap7) u = b`` on a slab that is periodic and decomposed
in ``(y, x)`` and local in z, with the zero z boundary (``u = 0`` above and
below the slab).  The operator is one ``CartesianGrid.make_stencil3d``: a
``(3, 3, 3)`` table with the seven taps of the 3-D Laplacian.
``gershgorin_bounds`` gives ``1 <= lambda <= 1 + 12 nu``, so the operator
is positive definite and ``make_cg().solve`` runs as for the 2-D stencil.

    python examples/stencil3d_poisson_cg.py
    python -m mpi4jax_amd.run -n 2 examples/stencil3d_poisson_cg.py
"""

import argparse
import math

import torch

import os as _os, sys as _sys
_sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))

import mpi4jax_amd as m
from mpi4jax_amd.parallel import CartesianGrid


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--size", type=int, default=64,
                   help="global interior cells per horizontal axis")
    p.add_argument("--nz", type=int, default=16)
    p.add_argument("--nu", type=float, default=2.0)
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
    z = (torch.arange(args.nz, dtype=torch.float64) + 0.5) / args.nz
    shape = (args.nz, by + 2, bx + 2)

    k = torch.zeros(3, 3, 3, dtype=torch.float64)
    for o in ((0, 1, 1), (2, 1, 1), (1, 0, 1), (1, 2, 1), (1, 1, 0),
              (1, 1, 2)):
        k[o] = -args.nu
    k[1, 1, 1] = 1.0 + 6.0 * args.nu
    st = grid.make_stencil3d(shape, torch.float64, device, k)
    lo, hi = st.gershgorin_bounds()
    assert lo == 1.0 and hi == 1.0 + 12.0 * args.nu

    b = torch.zeros(shape, dtype=torch.float64, device=device)
    b[:, 1:-1, 1:-1] = torch.exp(
        -((z[:, None, None] - 0.5) ** 2 + (y[None, :, None] - 0.5) ** 2
          + (x[None, None, :] - 0.5) ** 2) / 0.02).to(device)

    u, info = st.make_cg().solve(b, rtol=args.rtol, maxiter=2000)
    assert info.converged, f"no convergence in {info.iterations}"
    res = st.apply(u).sub_(b)  # the true residual, not the recurrence's
    true = math.sqrt(st.dot(res, res).item()) / info.rhs_norm
    assert true < 10 * args.rtol, f"true residual {true:.2e}"
    # the operator is an M-matrix and b >= 0: so is u, and sum(u) < sum(b)
    # because the zero boundary in z lets heat out
    tot = [m.allreduce(f[:, 1:-1, 1:-1].sum(), m.SUM, comm=comm).item()
           for f in (u, b)]
    low = m.allreduce(u[:, 1:-1, 1:-1].min(), m.MIN, comm=comm).item()
    assert low > -1e-12 and 0 < tot[0] < tot[1], (low, tot)
    if comm.rank == 0:
        print(f"n={args.size} nz={args.nz} nu={args.nu} device={device}: "
              f"{info.iterations} CG iterations, true residual {true:.1e}")
        print(f"OK: 3-D Helmholtz solved over {comm.size} rank(s)")


if __name__ == "__main__":
    main()
