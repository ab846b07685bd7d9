"""examples/stencil_chebyshev_diffusion.py runs on the CPU with 1 and 2
ranks, conserves the total and reaches a small true residual (the example
asserts both itself) in the number of iterations known beforehand."""

import math
import re
import subprocess
import sys

import pytest

from test_halo_exchanger import ENV, REPO


@pytest.mark.parametrize("n", [1, 2])
def test_stencil_chebyshev_example(n):
    cmd = [sys.executable, "examples/stencil_chebyshev_diffusion.py",
           "--size", "24", "--nz", "2", "--steps", "4", "--device", "cpu"]
    if n > 1:
        cmd = [sys.executable, "-m", "mpi4jax_amd.run", "-n", str(n)] + cmd[1:]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300,
                         env=ENV, cwd=REPO)
    assert res.returncode == 0, res.stderr + res.stdout
    assert f"OK: 4 implicit steps over {n} rank(s)" in res.stdout
    drift = float(re.search(r"total drift (\S+),", res.stdout).group(1))
    worst = float(re.search(r"true residual (\S+),", res.stdout).group(1))
    iters = int(re.search(r"(\d+) Chebyshev iterations", res.stdout).group(1))
    assert "bounds (1, 33)" in res.stdout
    assert drift < 1e-9 and worst < 1e-9
    # nu = 4: bounds (1, 33), sigma = 17 / 16, and the smallest k with
    # 1 / T_k(sigma) <= 1e-10, whatever the decomposition
    a = math.acosh(17 / 16)
    k = math.ceil(math.acosh(1e10) / a)
    assert 1 / math.cosh(k * a) <= 1e-10 < 1 / math.cosh((k - 1) * a)
    assert iters == 4 * k
