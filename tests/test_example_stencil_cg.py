"""examples/stencil_cg_diffusion.py runs on the CPU with 1 and 2 ranks,
conserves the total and reaches a small true residual (the example asserts
both itself)."""

import re
import subprocess
import sys

import pytest

from test_halo_exchanger import ENV, REPO


@pytest.mark.parametrize("n", [1, 2])
def test_stencil_cg_example(n):
    cmd = [sys.executable, "examples/stencil_cg_diffusion.py", "--size",
           "24", "--nz", "2", "--steps", "4", "--device", "cpu"]
    if n > 1:
        cmd = [sys.executable, "-m", "mpi4jax_amd.run", "-n", str(n)] + cmd[1:]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300,
                         env=ENV, cwd=REPO)
    assert res.returncode == 0, res.stderr + res.stdout
    assert f"OK: 4 implicit steps over {n} rank(s)" in res.stdout
    drift = float(re.search(r"total drift (\S+),", res.stdout).group(1))
    worst = float(re.search(r"true residual (\S+),", res.stdout).group(1))
    iters = int(re.search(r"(\d+) CG iterations", res.stdout).group(1))
    assert drift < 1e-9 and worst < 1e-9
    # nu = 4 is 16 times the explicit limit: CG must really iterate, and
    # the decomposition must not change the count
    assert 4 * 10 < iters <= 4 * 60
