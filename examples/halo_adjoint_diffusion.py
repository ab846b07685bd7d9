"""Gradient through a wide-stencil time loop: recover an initial field.

K explicit steps of the fourth-order diffusion stencil of
``wide_stencil_diffusion.py`` (halo ``width=2``) run under
``HaloExchanger.exchange_ad``, the differentiable halo exchange.  The loss
is ``||u_K - target||^2`` summed over all ranks; ``backward()`` carries it
back through the K exchanges — each one's backward pass is the exchange's
adjoint, a scatter-add with the message directions reversed — to the
gradient with respect to the initial field.  A few steps of gradient
descent on the initial field lower the loss.

    python examples/halo_adjoint_diffusion.py
    python -m mpi4jax_amd.run -n 2 examples/halo_adjoint_diffusion.py

The backward pass is a collective: every rank calls ``backward()``, which
is what happens when every rank runs this same program.
"""

import argparse

import torch
import torch.nn.functional as F

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


def forward(ex, interior, steps):
    """``steps`` diffusion steps from the interior cells ``interior``;
    returns the final interior.  Out of place, so autograd can follow."""
    for _ in range(steps):
        u = ex.exchange_ad(F.pad(interior, (W, W, W, W)))
        interior = u[:, W:-W, W:-W] + 0.1 * laplacian4(u)
    return interior


def bump(y, x, cy, cx):
    return torch.exp(-((y[:, None] - cy) ** 2 + (x[None, :] - cx) ** 2)
                     / 0.01)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--size", type=int, default=64,
                   help="global interior cells per horizontal axis")
    p.add_argument("--nz", type=int, default=2)
    p.add_argument("--steps", type=int, default=8,
                   help="diffusion steps K inside the loss")
    p.add_argument("--descent", type=int, default=5,
                   help="gradient-descent steps on the initial field")
    p.add_argument("--lr", type=float, default=0.4)
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

    ex = grid.make_halo_exchanger((args.nz, by + 2 * W, bx + 2 * W),
                                  torch.float64, device, width=W)

    # the target is the diffused image of a bump the descent never sees
    truth = (z * bump(y, x, 0.5, 0.5)).to(device)
    with torch.no_grad():
        target = forward(ex, truth, args.steps)

    # start from a displaced, weaker bump
    u0 = (0.5 * z * bump(y, x, 0.4, 0.6)).to(device).requires_grad_()

    losses = []
    for it in range(args.descent + 1):
        local = ((forward(ex, u0, args.steps) - target) ** 2).sum()
        loss = m.allreduce(local, m.SUM, comm=comm)
        losses.append(loss.item())
        if it == args.descent:
            break
        u0.grad = None
        loss.backward()  # K halo adjoints, on every rank
        with torch.no_grad():
            u0 -= args.lr * u0.grad

    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    if comm.rank == 0:
        print(f"n={args.size} nz={args.nz} K={args.steps} device={device}")
        print(f"loss before: {losses[0]:.6e}")
        print(f"loss after {args.descent} descent steps: {losses[-1]:.6e}")
        print(f"OK: gradient through {args.steps} halo exchanges over "
              f"{comm.size} rank(s)")


if __name__ == "__main__":
    main()
