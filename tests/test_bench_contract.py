"""Pin the driver-facing bench.py contract on CPU.

The driver runs ``python bench.py --gpus N --steps K --warmup W`` (N>1
under torch.distributed.run) and parses ONE JSON line from rank 0; it
also relies on ``--preflight`` never being broken so the first multi-GPU
contact cannot die on schedule bugs.
"""

import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, timeout=420):
    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    return subprocess.run(
        [sys.executable] + args, cwd=REPO, env=env, timeout=timeout,
        capture_output=True, text=True,
    )


def test_preflight_world2():
    r = _run(["-m", "torch.distributed.run", "--nnodes=1",
              "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
              "--master-port", "29591", "bench.py", "--preflight"])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PREFLIGHT_OK world_size=2" in r.stdout


def test_bench_json_contract_cpu():
    r = _run(["bench.py", "--steps", "4", "--warmup", "1",
              "--nx", "360", "--ny", "180"])
    assert r.returncode == 0, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d["metric"] == "shallow_water_steps_per_sec"
    assert d["steps"] == 4 and d["warmup"] == 1
    assert d["n_gpus"] == 1
    assert d["higher_is_better"] is True
    assert d["scaling"] == "strong"
    assert d["data"] == "synthetic"
    assert "sec_per_model_day" in d["config"]
    assert d["value"] > 0


def test_bench_dump_outputs_cpu(tmp_path):
    """--dump-outputs writes the last timed step's state as float .npy
    files, identical from run to run; an odd --steps is honoured."""
    import numpy as np

    dumps = []
    for sub in ("a", "b"):
        out = tmp_path / sub
        r = _run(["bench.py", "--steps", "3", "--warmup", "1",
                  "--nx", "360", "--ny", "180", "--dump-outputs", str(out)])
        assert r.returncode == 0, r.stdout + r.stderr
        line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
        d = json.loads(line)
        assert d["steps"] == 3 and d["ms_per_step"] > 0
        assert "allreduce_256MiB_bf16" not in d["config"]  # needs --full
        dumps.append({f: np.load(out / f) for f in sorted(os.listdir(out))})
    a, b = dumps
    assert sorted(a) == [n + ".npy" for n in ("dh", "du", "dv", "h", "u", "v")]
    for name, arr in a.items():
        assert arr.dtype in (np.float32, np.float64), (name, arr.dtype)
        # the local arrays as the step returns them: domain + halo ring
        assert arr.shape == (182, 362) and np.isfinite(arr).all(), name
        assert np.array_equal(arr, b[name]), name
    assert a["h.npy"].std() > 0


@pytest.mark.gpu
def test_bench_odd_steps_and_dump_gpu(tmp_path):
    """A plain run with an odd --steps (graph capture takes even counts
    only, the last step runs eagerly) times exactly that many steps,
    carries no comm configs, and dumps the finite fused-path state."""
    import numpy as np

    r = _run(["bench.py", "--gpus", "1", "--steps", "11", "--warmup", "2",
              "--nx", "360", "--ny", "180", "--dump-outputs", str(tmp_path)])
    assert r.returncode == 0, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d["steps"] == 11 and d["ms_per_step"] > 0
    assert d["config"]["fused_kernels"] is True
    assert "allreduce_256MiB_bf16" not in d["config"]
    for name in ("h", "u", "v", "dh", "du", "dv"):
        arr = np.load(tmp_path / (name + ".npy"))
        assert arr.dtype == np.float32 and arr.shape == (182, 362), name
        assert np.isfinite(arr).all(), name


@pytest.mark.gpu
def test_bench_comm_configs_gpu():
    """On a GPU box the ``--full`` line must carry every BASELINE comm
    config, n_gpus-labeled, with the N=1 local-copy caveat."""
    r = _run(["bench.py", "--full", "--steps", "20", "--warmup", "5"],
             timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    cfg = d["config"]
    ar = cfg["allreduce_256MiB_bf16"]
    assert "error" not in ar, ar
    assert ar["n_gpus"] == 1 and "note" in ar
    bis = cfg["bisection_1GiB_bf16"]
    assert "error" not in bis, bis
    assert bis["alltoall"]["n_gpus"] == 1
    assert bis["allgather"]["n_gpus"] == 1
    ga = cfg["grad_allreduce_256MiB_bf16"]
    assert "error" not in ga, ga
    assert ga["ms"] > 0
