"""bench.py's multi-process contract on the C++ engine, on the CPU backend (host TCP ring): the
torch.distributed launcher starts one bench.py per rank, each runs the C++ trainer as a child with
--dp, rank 0 prints one JSON line with the whole job's images/sec; when any rank's child fails,
every rank falls back to the Python engine (agreement over a CPU gloo group)."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "dcnn_amd", "bin", "tiny_imagenet_resnet18")


@pytest.fixture(scope="module")
def built():
    if not (os.path.exists(EXE) and torch.cuda.is_available()):
        from dcnn_amd import _build
        _build.build_host()


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _torchrun(world, extra_env=None):
    env = dict(os.environ, OMP_NUM_THREADS="2", **(extra_env or {}))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1", "--master-port", str(_port()), os.path.join(ROOT, "bench.py"),
           "--gpus", str(world), "--steps", "1", "--warmup", "1", "--batch", "2", "--device", "cpu",
           "--dtype", "fp32", "--engine", "native"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    return r, lines


def test_bench_native_two_ranks_cpu(built):
    r, lines = _torchrun(2)
    assert r.returncode == 0, r.stderr[-3000:]
    assert len(lines) == 1, r.stdout  # rank 0 only
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["global_batch"] == 4
    assert d["config"]["engine"].startswith("native") and d["config"]["data_plane"] == "tcp"
    assert d["config"]["dp_buckets"] >= 2 and d["value"] > 0


@pytest.mark.parametrize("engine", ["native", "python"])
def test_bench_dump_outputs_cpu(built, tmp_path, engine):
    """--dump-outputs: loss.npy (float64, the result line's final_loss) and params.npy (float32,
    every parameter of ResNet-18) after --steps timed steps; a second run with the same arguments
    trains on the same inputs from the same weights (CPU backend: the same bits); --full is accepted.
    The parameters are those the last timed step left: a run of one step fewer leaves other values
    (Adam moves every parameter with a non-zero gradient by about the learning rate per step).
    --warmup 0: the C++ trainer runs one warm-up step and the line says so."""
    import numpy as np
    outs = []
    for name, steps, warmup, extra in (("a", 2, 1, []), ("b", 2, 1, ["--full"]), ("c", 1, 0, [])):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
               str(warmup), "--batch", "2", "--device", "cpu", "--dtype", "fp32", "--engine", engine,
               "--dump-outputs", str(tmp_path / name)] + extra
        r = subprocess.run(cmd, cwd=tmp_path, env=dict(os.environ, OMP_NUM_THREADS="2"), stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout
        d = json.loads(lines[0])
        assert d["steps"] == steps and d["ms_per_step"] > 0
        assert d["warmup"] == (max(1, warmup) if engine == "native" else warmup)
        assert abs(d["value"] - 2 * 1000.0 / d["ms_per_step"]) < 0.02 * d["value"]
        assert sorted(os.listdir(tmp_path / name)) == ["loss.npy", "params.npy"]
        loss, params = np.load(tmp_path / name / "loss.npy"), np.load(tmp_path / name / "params.npy")
        assert loss.dtype == np.float64 and loss.shape == (1,) and abs(loss[0] - d["config"]["final_loss"]) < 1e-4
        assert params.dtype == np.float32 and params.shape == (11258088,) and np.isfinite(params).all()
        outs.append((loss, params))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert outs[2][0][0] != outs[0][0][0] and np.mean(outs[2][1] != outs[0][1]) > 0.5


def test_bench_native_failure_falls_back_everywhere(built):
    r, lines = _torchrun(2, {"DCNN_BENCH_FAULT_RANK": "1", "DCNN_DIST_TIMEOUT": "5"})
    # rank 1 fails before its rendezvous, rank 0 gives up after DCNN_DIST_TIMEOUT; --engine native was
    # asked explicitly, so the agreed failure is an error (auto would run the Python engine)
    assert r.returncode != 0
    assert "C++ engine failed" in r.stderr
