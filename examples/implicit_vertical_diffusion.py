"""Backward-Euler vertical diffusion with a diffusivity that differs in
every column and changes every step.

Each step solves ``(I - dt dz kappa dz) T' = T`` on every ``(j, i)`` column
of a ``(nz, ny, nx)`` tracer: one tridiagonal system per column, with
``kappa(z, y, x)`` on the cell interfaces (a surface mixed layer whose depth
moves with time over a weak background) and no flux through the surface or
the bottom.  The sea floor is uneven: a column's cells below its depth are
identity rows, and the interface above them carries no flux.  The bands
are new every step, so the solve goes through ``solve_bands``: factorise
and solve in one launch, with no host read.

No flux leaves a column, so its tracer content is conserved; diffusion
never raises the maximum or lowers the minimum.  Both are checked.

    python examples/implicit_vertical_diffusion.py
"""

import argparse
import math

import torch

import os as _os, sys as _sys
_sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))

import mpi4jax_amd as m
from mpi4jax_amd.parallel import CartesianGrid


def bands(step, depth, dt, nz, ny, nx, device):
    """``lower``, ``diag``, ``upper`` of ``I - dt dz kappa dz`` (dz = 1)."""
    z = torch.arange(1, nz, dtype=torch.float64, device=device)
    y = torch.arange(ny, dtype=torch.float64, device=device)
    x = torch.arange(nx, dtype=torch.float64, device=device)
    # mixed-layer depth: a wave that travels in x and deepens with y
    mld = 2.0 + 0.25 * nz * (1.0 + torch.sin(
        2.0 * math.pi * (x[None, :] / nx + 0.05 * step))) * (
            0.5 + y[:, None] / (2.0 * ny))
    # kappa on the interface between cells k - 1 and k, k = 1 .. nz - 1
    kappa = 1e-2 + 5.0 * torch.sigmoid(2.0 * (mld[None] - z[:, None, None]))
    kappa = kappa * (z[:, None, None] < depth[None])  # dry below the floor
    lower = torch.zeros(nz, ny, nx, dtype=torch.float64, device=device)
    upper = torch.zeros_like(lower)
    lower[1:] = -dt * kappa
    upper[:-1] = -dt * kappa
    return lower, 1.0 - lower - upper, upper


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--size", type=int, default=48)
    p.add_argument("--nz", type=int, default=24)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--dt", type=float, default=2.0)
    p.add_argument("--device", default=None)
    args = p.parse_args()

    m.init()
    device = args.device or ("cuda" if torch.cuda.is_available() else "cpu")
    grid = CartesianGrid(dims=(1, 1), periodic=(True, True))
    nz, ny, nx = args.nz, args.size, args.size
    g = torch.Generator().manual_seed(5)
    depth = torch.randint(nz // 2, nz + 1, (ny, nx), generator=g).to(device)
    wet = (torch.arange(nz, device=device)[:, None, None] < depth[None])
    # a warm surface over a cold interior, two tracers (a batch of two)
    profile = torch.exp(-torch.arange(nz, dtype=torch.float64) / 3.0)
    t = torch.stack([profile[:, None, None].expand(nz, ny, nx),
                     torch.rand(nz, ny, nx, generator=g, dtype=torch.float64)])
    t = (t.to(device) * wet).contiguous()
    solver = grid.make_tridiagonal_solver(
        t.shape, torch.float64, device,
        *bands(0, depth, args.dt, nz, ny, nx, device))
    content, top, bottom = t.sum(dim=1), t.amax(), t.amin()
    spread = t[0].var(dim=0).mean().item()
    for step in range(args.steps):
        t = solver.solve_bands(
            *bands(step, depth, args.dt, nz, ny, nx, device), t)
    drift = ((t.sum(dim=1) - content).abs().max() / content.abs().max()).item()
    assert drift < 1e-12, f"column content drifted by {drift:.2e}"
    assert t.amax() <= top + 1e-12 and t.amin() >= bottom - 1e-12
    assert (t * ~wet).abs().max() == 0.0, "a dry cell changed"
    after = t[0].var(dim=0).mean().item()
    assert after < 0.5 * spread, (spread, after)
    print(f"OK: {args.steps} implicit steps of {ny * nx} columns x {nz} "
          f"levels on {device}; vertical variance {spread:.4f} -> "
          f"{after:.4f}, column content drift {drift:.1e}")


if __name__ == "__main__":
    main()
