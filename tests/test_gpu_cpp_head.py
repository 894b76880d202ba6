"""The C++ engine's fused classifier head (Sequential's fusion pass: the average pool runs
gpu_ops::head_fwd, Dense::backward runs gpu_ops::head_bwd) against the six-launch path
(DCNN_HEAD_FUSE=0), with the C++ CPU backend (fp32) as the reference: host_api_parity grads on the
same weights and batch, the way tests/test_cpp_host_blocks.py compares fusion switches.

Per parameter: rel-L2(fused GPU, CPU) <= 1.5 x rel-L2(unfused GPU, CPU) + 1e-4; the classifier's
weight and bias gradients are non-zero; and, since the fused kernels keep the separate kernels'
summation order, every gradient is bit-identical to the unfused run's. Then one short captured
training run each way: the final losses agree to 1e-2 relative, and are in fact equal."""
import json
import os
import subprocess

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dcnn_amd", "bin")
NAMES = ("host_api_parity", "tiny_imagenet_resnet18")


@pytest.fixture(scope="module")
def bins():
    have = all(os.path.exists(os.path.join(BIN, n)) for n in NAMES)
    if not (have and torch.cuda.is_available()):
        from dcnn_amd import _build
        _build.build_host()
    return {n: os.path.join(BIN, n) for n in NAMES}


def _run(cmd, cwd, env=None, timeout=600):
    r = subprocess.run(cmd, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:]
    return r.stdout


def _grads(bins, tmp_path, model, batch, tag, device, fuse=None):
    from dcnn_amd.nn.sequential import load_tensor
    env = dict(os.environ)
    if fuse is not None:
        env["DCNN_HEAD_FUSE"] = fuse
    out = _run([bins["host_api_parity"], "grads", model, str(batch), f"{tag}.bin", "--device", device], tmp_path, env)
    names = [l.split()[1:] for l in out.splitlines() if l.startswith("params")][0]
    with open(tmp_path / f"{tag}.bin", "rb") as f:
        return names, [load_tensor(f).double() for _ in names]


def _rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


@pytest.mark.parametrize("model,batch", [("resnet18_tiny_imagenet", 64), ("resnet50_tiny_imagenet", 32)])
def test_cpp_head_fusion_gradients_match_unfused(bins, tmp_path, model, batch):
    names, cpu = _grads(bins, tmp_path, model, batch, "cpu", "CPU")
    names1, g1 = _grads(bins, tmp_path, model, batch, "g1", "GPU", "1")
    names0, g0 = _grads(bins, tmp_path, model, batch, "g0", "GPU", "0")
    assert names == names1 == names0 and len(names) > 40
    bad = []
    for n, a, b, c in zip(names, g1, g0, cpu):
        e1, e0 = _rel(a, c), _rel(b, c)
        print(f"{n}: fused {e1:.3e}, unfused {e0:.3e}")
        if not e1 <= 1.5 * e0 + 1e-4:
            bad.append((n, e1, e0))
    assert not bad, bad
    # the fused kernels keep the separate kernels' summation order and rounding points
    for n, a, b in zip(names, g1, g0):
        assert torch.equal(a, b), (n, float((a - b).abs().max()), float(b.abs().max()))
    # the classifier's weights and bias: the last two parameters
    assert float(g1[-2].abs().max()) > 0 and float(g1[-1].abs().max()) > 0
    assert tuple(g1[-2].shape[:2]) == (200, 512 if "18" in model else 2048)


def test_cpp_head_fusion_training_loss_matches_unfused(bins, tmp_path):
    loss = {}
    for fuse in ("1", "0"):
        out = _run([bins["tiny_imagenet_resnet18"], "--device", "GPU", "--bench", "--batch", "64", "--steps", "6",
                    "--warmup", "2", "--loss", "softmax_ce"], tmp_path, dict(os.environ, DCNN_HEAD_FUSE=fuse))
        loss[fuse] = float(json.loads(out.strip().splitlines()[-1])["loss"])
    print(f"final loss: fused {loss['1']!r}, unfused {loss['0']!r}")
    assert loss["1"] == loss["1"] and loss["0"] == loss["0"]
    assert abs(loss["1"] - loss["0"]) <= 1e-2 * abs(loss["0"])
    assert loss["1"] == loss["0"]  # (bit-identical gradients: the same training run)
