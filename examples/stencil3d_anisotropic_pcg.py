"""Anisotropic 3-D Helmholtz solve: plain CG against vertical-line
preconditioned CG.

Solves ``(I - lap_h - az * lap_z) u = b`` on thin layers over a wide
horizontal grid: decomposed and periodic in ``(y, x)``, local and periodic
in z.  With ``az`` large the z coupling dominates, plain CG's iteration
count grows with ``az``, and ``make_cg("zline")``, which solves the
vertical tridiagonal part of the operator exactly in every iteration,
stays flat.  The preconditioner needs no communication: z is never
decomposed.

    python examples/stencil3d_anisotropic_pcg.py
    python -m mpi4jax_amd.run -n 2 examples/stencil3d_anisotropic_pcg.py
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
    p.add_argument("--size", type=int, default=32,
                   help="global interior cells per horizontal axis")
    p.add_argument("--nz", type=int, default=8)
    p.add_argument("--rtol", type=float, default=1e-5)
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
    shape = (args.nz, by + 2, bx + 2)
    g = torch.Generator().manual_seed(11 + comm.rank)
    b = torch.zeros(shape, dtype=torch.float32)
    b[:, 1:-1, 1:-1] = torch.randn(args.nz, by, bx, generator=g)
    b = b.to(device)

    counts = {}
    for az in (1.0, 16.0, 100.0):
        k = torch.zeros(3, 3, 3, dtype=torch.float64)
        k[0, 1, 1] = k[2, 1, 1] = -az
        k[1, 0, 1] = k[1, 2, 1] = k[1, 1, 0] = k[1, 1, 2] = -1.0
        k[1, 1, 1] = 1.0 + 2.0 * az + 4.0
        st = grid.make_stencil3d(shape, torch.float32, device, k,
                                 z_boundary="periodic")
        for name, pre in (("cg", None), ("pcg", "zline")):
            u, info = st.make_cg(pre).solve(b, rtol=args.rtol, maxiter=2000,
                                            check_every=1)
            assert info.converged, f"{name}: no convergence at az={az}"
            res = st.apply(u).sub_(b)  # the true residual
            true = math.sqrt(st.dot(res, res).item()) / info.rhs_norm
            assert true < 10 * args.rtol, f"{name}: true residual {true:.2e}"
            counts[az, name] = info.iterations
        if comm.rank == 0:
            print(f"az={az:5.0f}: CG {counts[az, 'cg']:4d} iterations, "
                  f"line-preconditioned CG {counts[az, 'pcg']:4d}")
    assert counts[100.0, "pcg"] * 2 <= counts[100.0, "cg"]
    if comm.rank == 0:
        print(f"OK: anisotropic solves on {device} over {comm.size} rank(s)")


if __name__ == "__main__":
    main()
