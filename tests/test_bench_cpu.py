"""bench.py's distributed logic end to end on CPU: gloo ranks launched by
torch.distributed.run or by bench.py itself (``--gpus N`` with no launcher
around it), a tiny graph on the PyTorch path; rank 0 prints the one JSON line
of the driver contract (the GPU run differs only in device/backend)."""
import json
import os

import numpy as np
import pytest
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


# 4: halo path; 8: the driver's node size (halo plans, train-column slots and row blocks
# at the shapes of the 8-GPU scaling run)
@pytest.mark.parametrize("nproc,launcher", [(2, "torchrun"), (2, "self"), (4, "self"), (8, "torchrun")])
def test_bench_gloo_ranks_print_one_json_line(nproc, launcher):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["OMP_NUM_THREADS"] = "1" if nproc > 4 else "2"
    args = ["bench.py", "--gpus", str(nproc), "--steps", "2", "--warmup", "1", "--device", "cpu",
            "--scale", "0.002", "--hidden", "64", "--full"]
    if launcher == "torchrun":
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
               "--master-addr", "127.0.0.1", "--master-port", str(_free_port())] + args
    else:
        cmd = [sys.executable] + args
    res = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout
    out = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                "scaling", "vs_baseline", "dtype", "data", "config", "val_acc"):
        assert key in out, key
    assert out["n_gpus"] == nproc and out["steps"] == 2 and out["warmup"] == 1
    assert out["value"] > 0 and abs(out["value"] * out["ms_per_step"] / 1000.0 - 1.0) < 1e-3
    assert out["config"]["parallelism"] == "graph-rowpart%d" % nproc
    # the process group that ran it (checked by the pre-timing collective self-test)
    assert out["backend"] == "gloo" and out["world_size"] == nproc


def _plain(tmp_path, name, steps=2):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["OMP_NUM_THREADS"] = "1"          # one thread: index_add_ sums in one order
    d = tmp_path / name
    res = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                          "--device", "cpu", "--scale", "0.002", "--hidden", "64", "--dump-outputs", str(d)],
                         cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout
    return json.loads(lines[0]), {p.name[:-4]: np.load(p) for p in d.glob("*.npy")}


def test_bench_plain_run_dumps_the_last_step(tmp_path):
    """A plain run (no ``--full``) skips the evaluation pass and still prints the headline
    keys; ``--dump-outputs`` writes the last timed epoch's arrays, equal from run to run
    with the same arguments, after warm-up + ``--steps`` epochs by the trainer's count."""
    out, arr = _plain(tmp_path, "a")
    out2, arr2 = _plain(tmp_path, "b")
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "train_loss"):
        assert key in out, key
    assert out["full"] is False and "val_acc" not in out and "test_acc" not in out
    assert out["steps"] == 2 and out["epochs_trained"] == 3         # the trainer's own count: 1 + 2
    assert set(arr) == {"train_stats", "grads", "params", "adam_m", "adam_v"}
    n_params = 100 * 64 + 64 + 64 * 47 + 47
    total = 0
    for name, x in arr.items():
        assert x.dtype == np.float32 and np.all(np.isfinite(x)), name
        assert x.shape == ((4,) if name == "train_stats" else (n_params,)), (name, x.shape)
        assert np.array_equal(x, arr2[name]), name              # same arguments: same arrays
        total += x.nbytes
    assert total <= 64 << 20
    assert arr["train_stats"][0] > 0                            # the loss sum behind train_loss
    assert np.any(arr["grads"] != 0) and np.any(arr["adam_v"] != 0)


def test_bench_rejects_rank_count_mismatch():
    """--gpus must equal the launcher's world size (a silent 1-rank run is an error)."""
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", OMP_NUM_THREADS="2")
    res = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--device", "cpu", "--scale", "0.002"],
                         cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         timeout=300)
    assert res.returncode != 0 and "launcher started 1 ranks" in res.stderr
