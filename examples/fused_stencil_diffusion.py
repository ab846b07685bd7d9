"""Fourth-order diffusion with the fused halo stencil operator.

The diffusion of ``wide_stencil_diffusion.py`` written with
``CartesianGrid.make_stencil``: one step is ``u <- u + 0.1 * lap4(u)``, a
constant-coefficient stencil of radius 2, so the weights are the identity
plus 0.1 times the fourth-order Laplacian and one ``apply`` is a whole
step — halo exchange included.  On one GPU that is one kernel launch per
step; across ranks it is the exchanger's pack launch, one RCCL group and
one stencil launch.  Two buffers ping-pong through ``out=``.

The second half takes one gradient through K steps with ``apply_ad``,
whose backward pass is the operator's native adjoint, and runs a few steps
of gradient descent on the initial field, as ``halo_adjoint_diffusion.py``
does with ``exchange_ad`` and slicing.

    python examples/fused_stencil_diffusion.py
    python -m mpi4jax_amd.run -n 2 examples/fused_stencil_diffusion.py

The periodic problem conserves the field's total, which is checked across
all ranks.  The backward pass is a collective: every rank calls
``backward()``.
"""

import argparse
import time

import torch
import torch.nn.functional as F

import os as _os, sys as _sys
_sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))

import mpi4jax_amd as m
from mpi4jax_amd.parallel import CartesianGrid

W = 2  # halo width of the fourth-order stencil


def diffusion_weights(nu=0.1):
    """Identity + nu * (fourth-order 5+5-point Laplacian), as a 5x5
    table; entry [a][b] multiplies the cell at offset (a - 2, b - 2)."""
    k = torch.zeros(5, 5, dtype=torch.float64)
    axis = torch.tensor([-1.0, 16.0, -30.0, 16.0, -1.0],
                        dtype=torch.float64) / 12.0
    k[2, :] += nu * axis
    k[:, 2] += nu * axis
    k[2, 2] += 1.0
    return k


def bump(y, x, cy, cx):
    return torch.exp(-((y[:, None] - cy) ** 2 + (x[None, :] - cx) ** 2)
                     / 0.01)


def forward(st, interior, steps):
    """``steps`` diffusion steps under autograd; returns the interior."""
    u = F.pad(interior, (W, W, W, W))
    for _ in range(steps):
        u = st.apply_ad(u)
    return u[:, W:-W, W:-W]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--size", type=int, default=128,
                   help="global interior cells per horizontal axis")
    p.add_argument("--nz", type=int, default=4)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--grad-steps", type=int, default=8,
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

    shape = (args.nz, by + 2 * W, bx + 2 * W)
    st = grid.make_stencil(shape, torch.float64, device, diffusion_weights())

    # ---- the time loop: one apply per step, ping-pong through out=
    u = torch.zeros(shape, dtype=torch.float64, device=device)
    v = torch.zeros_like(u)
    u[:, W:-W, W:-W] = (z * bump(y, x, 0.5, 0.5)).to(device)
    total0 = m.allreduce(u[:, W:-W, W:-W].sum(), m.SUM, comm=comm).item()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        st.apply(u, out=v)
        u, v = v, u
    if device == "cuda":
        torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    total = m.allreduce(u[:, W:-W, W:-W].sum(), m.SUM, comm=comm).item()
    peak = m.allreduce(u[:, W:-W, W:-W].max(), m.MAX, comm=comm).item()
    drift = abs(total - total0) / abs(total0)
    assert drift < 1e-12, f"total drifted by {drift:.2e}"
    assert peak < float(args.nz), "diffusion must lower the peak"

    # ---- a gradient through K steps: recover an initial field
    truth = (z * bump(y, x, 0.5, 0.5)).to(device)
    with torch.no_grad():
        target = forward(st, truth, args.grad_steps)
    u0 = (0.5 * z * bump(y, x, 0.4, 0.6)).to(device).requires_grad_()
    losses = []
    for it in range(args.descent + 1):
        local = ((forward(st, u0, args.grad_steps) - target) ** 2).sum()
        loss = m.allreduce(local, m.SUM, comm=comm)
        losses.append(loss.item())
        if it == args.descent:
            break
        u0.grad = None
        loss.backward()  # K stencil adjoints, on every rank
        with torch.no_grad():
            u0 -= args.lr * u0.grad
    assert all(b < a for a, b in zip(losses, losses[1:])), losses

    if comm.rank == 0:
        print(f"n={args.size} nz={args.nz} device={device}: peak {peak:.6f}, "
              f"total drift {drift:.1e}, {wall:.3f}s")
        print(f"loss before: {losses[0]:.6e}")
        print(f"loss after {args.descent} descent steps: {losses[-1]:.6e}")
        print(f"OK: {args.steps} fused steps and a gradient through "
              f"{args.grad_steps} over {comm.size} rank(s)")


if __name__ == "__main__":
    main()
