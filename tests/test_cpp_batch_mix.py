"""Mixup / CutMix and the soft-target loss in the C++ host API (csrc/host: dcnn::BatchMixer,
cpu_ops / gpu_ops mix_plan / mix_batch, loss kind 6, TrainGraph with a dense target, the
dcnn_c_mix_* / dcnn_c_soft_loss* C ABI), through ctypes on libdcnn.so and examples/cpp/host_api_parity
like tests/test_cpp_drop_path.py, checked against the Python front end."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dcnn_amd", "bin")
LIB = os.path.join(ROOT, "dcnn_amd", "libdcnn.so")
MODEL = "convnext_two_block"
P = ctypes.c_void_p
TOL = dict(rtol=1e-5, atol=1e-7)  # the native CPU backend's, tests/test_cpp_host_blocks.py
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def parity():
    exe = os.path.join(BIN, "host_api_parity")
    if not (os.path.exists(exe) and os.path.exists(LIB)):
        from dcnn_amd import _build
        _build.build_host()
    return exe


def _lib():
    L = ctypes.CDLL(LIB)
    L.dcnn_c_last_error.restype = ctypes.c_char_p
    for name in ("dcnn_c_mix_plan", "dcnn_c_mix_batch", "dcnn_c_mix_batch_host", "dcnn_c_soft_loss",
                 "dcnn_c_soft_loss_host"):
        getattr(L, name).restype = ctypes.c_int
    return L


def _run(cmd, cwd, timeout=300, ok=True):
    r = subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    if ok:
        assert r.returncode == 0, r.stdout[-3000:]
    return r


def _lines(out):
    return {l.split()[0]: l.split()[1:] for l in out.splitlines() if l.split()}


def _c_plan(L, seed, step, H, W, ma, ca, prob, sw):
    out = (ctypes.c_int * 6)()
    lam = ctypes.c_double()
    rc = L.dcnn_c_mix_plan(ctypes.c_uint64(seed), ctypes.c_uint64(step), ctypes.c_int(H), ctypes.c_int(W),
                           ctypes.c_double(ma), ctypes.c_double(ca), ctypes.c_double(prob), ctypes.c_double(sw), out,
                           ctypes.byref(lam))
    return rc, (out[0], lam.value, out[1], out[2], out[3], out[4])


def test_c_abi_plan_is_the_python_modules(parity):
    from dcnn_amd.ops import cpu
    L = _lib()
    for seed in (0, 7, (1 << 40) + 3):
        for step in (1, 2, 3, 50, 1000, 1 << 33):
            for H, W in ((5, 5), (32, 32), (64, 48)):
                for ma, ca, prob, sw in ((0.8, 1.0, 1.0, 0.5), (0.2, 0.0, 0.7, 0.5), (0.0, 1.0, 1.0, 0.1)):
                    rc, plan = _c_plan(L, seed, step, H, W, ma, ca, prob, sw)
                    assert rc == 0, L.dcnn_c_last_error().decode()
                    assert plan == cpu.mix_plan(seed, step, H, W, ma, ca, prob, sw)
    rc, _ = _c_plan(L, 0, 1, 8, 8, -0.5, 1.0, 1.0, 0.5)
    assert rc == -1 and "mixup_alpha -0.5" in L.dcnn_c_last_error().decode()


def _mix_cases():
    return [(4, (3, 5, 5), 10, 1, 0.3, (0, 0, 0, 0)), (5, (1, 28, 28), 3, 1, 0.9172, (0, 0, 0, 0)),
            (8, (3, 8, 8), 200, 2, 1 - 12 / 64, (2, 5, 0, 4)), (5, (3, 8, 8), 10, 2, 1 - 8 / 64, (7, 8, 0, 8)),
            (6, (3, 8, 8), 10, 0, 1.0, (0, 0, 0, 0)), (1, (3, 8, 8), 10, 1, 0.5, (0, 0, 0, 0))]


def _c_mix(fn, x, lab, tgt, mode, lam, box, K):
    B, C, H, W = x.shape
    return fn(P(x.data_ptr()), P(lab.data_ptr()), P(tgt.data_ptr()), ctypes.c_long(B), ctypes.c_long(C),
              ctypes.c_long(H), ctypes.c_long(W), ctypes.c_int(mode), ctypes.c_double(lam), (ctypes.c_int * 4)(*box),
              ctypes.c_long(K))


def test_c_abi_host_mix_batch_equals_python(parity):
    from dcnn_amd.ops import cpu
    L = _lib()
    for k, (B, row, K, mode, lam, box) in enumerate(_mix_cases()):
        g = torch.Generator().manual_seed(k)
        x = torch.randn((B,) + row, generator=g)
        lab = torch.randint(0, K, (B,), generator=g)
        xa, ta = x.clone(), torch.full((B, K), -7.0)
        xb, tb = x.clone(), torch.full((B, K), -7.0)
        cpu.mix_batch(xa, lab, ta, mode, lam, box, K)
        assert _c_mix(L.dcnn_c_mix_batch_host, xb, lab, tb, mode, lam, box, K) == 0, L.dcnn_c_last_error().decode()
        assert torch.equal(xa, xb) and torch.equal(ta, tb)
    assert _c_mix(L.dcnn_c_mix_batch_host, xb, lab, tb, 1, 1.5, (0, 0, 0, 0), K) == -1
    assert "lam 1.5" in L.dcnn_c_last_error().decode()


def _loss_inputs(N, C, seed=0):
    g = torch.Generator().manual_seed(seed + N + C)
    x = 3 * torch.randn(N, C, generator=g)
    lab = torch.randint(0, C, (N,), generator=g)
    t = torch.zeros(N, C)
    lam = torch.rand(N, generator=g)
    t[torch.arange(N), lab] += lam
    t[torch.arange(N), torch.randint(0, C, (N,), generator=g)] += 1 - lam
    return x, lab, t


def test_c_abi_host_soft_loss_equals_python(parity):
    from dcnn_amd.nn import SoftTargetCrossEntropyLoss
    L = _lib()
    for N, C in ((1, 3), (5, 10), (64, 200)):
        x, lab, t = _loss_inputs(N, C)
        for eps in (0.0, 0.1):
            for dense in (True, False):
                pl, pg, pc = SoftTargetCrossEntropyLoss(eps).loss_and_grad(x, t if dense else lab)
                grad = torch.full((N, C), -9.0)
                loss, cor = ctypes.c_double(), ctypes.c_long()
                rc = L.dcnn_c_soft_loss_host(P(x.data_ptr()), P(t.data_ptr()) if dense else None,
                                             None if dense else P(lab.data_ptr()), P(grad.data_ptr()), ctypes.c_long(N),
                                             ctypes.c_long(C), ctypes.c_float(eps), ctypes.byref(loss),
                                             ctypes.byref(cor))
                assert rc == 0, L.dcnn_c_last_error().decode()
                assert np.isclose(loss.value, float(pl), **TOL) and cor.value == int(pc)
                assert torch.allclose(grad, pg, **TOL)
    rc = L.dcnn_c_soft_loss_host(P(x.data_ptr()), None, P(lab.data_ptr()), P(grad.data_ptr()), ctypes.c_long(N),
                                 ctypes.c_long(C), ctypes.c_float(1.0), ctypes.byref(loss), ctypes.byref(cor))
    assert rc == -1 and "label_smoothing" in L.dcnn_c_last_error().decode()


def test_cpp_cpu_training_on_mixed_batches(parity, tmp_path):
    """dcnn::BatchMixer + LossFactory::create("soft_crossentropy", 0.1) on the CPU backend: finite
    losses that differ from the unmixed run's; the eager path refuses nothing."""
    (tmp_path / "snap").mkdir()
    a = _lines(_run([parity, "train", MODEL, "3", "6", "snap/a", "--mix"], tmp_path).stdout)
    b = _lines(_run([parity, "train", MODEL, "3", "6", "snap/b"], tmp_path).stdout)
    la, lb = [float(v) for v in a["losses"]], [float(v) for v in b["losses"]]
    assert len(la) == 3 and all(np.isfinite(la)) and la != lb


# ------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_c_abi_device_mix_batch_equals_python(parity):
    from dcnn_amd.ops import hip
    L = _lib()
    for k, (B, row, K, mode, lam, box) in enumerate(_mix_cases()):
        g = torch.Generator().manual_seed(k)
        x = torch.randn((B,) + row, generator=g).cuda()
        lab = torch.randint(0, K, (B,), generator=g).cuda()
        xa, ta = x.clone(), torch.full((B, K), -7.0, device="cuda")
        xb, tb = x.clone(), torch.full((B, K), -7.0, device="cuda")
        hip.mix_batch(xa, lab, ta, mode, lam, box, K)
        torch.cuda.synchronize()
        assert _c_mix(L.dcnn_c_mix_batch, xb, lab, tb, mode, lam, box, K) == 0, L.dcnn_c_last_error().decode()
        assert torch.equal(xa, xb) and torch.equal(ta, tb)
    assert _c_mix(L.dcnn_c_mix_batch, xb, lab, tb, 2, 0.5, (0, 9, 0, 4), K) == -1
    assert "[0, 9)" in L.dcnn_c_last_error().decode()


@pytest.mark.gpu
def test_c_abi_device_soft_loss_equals_python(parity):
    """The C++ engine's loss runs on bf16 logits: the Python front end's kernel on the same bf16 tensor
    is the same launch, so the bits agree; and both are within the bf16 bound of the CPU backend."""
    from dcnn_amd.nn import SoftTargetCrossEntropyLoss
    L = _lib()
    for N, C in ((4, 10), (5, 65), (64, 200)):
        x, lab, t = _loss_inputs(N, C)
        xg, labg, tg = x.to(BF16).cuda(), lab.cuda(), t.cuda()
        for eps in (0.0, 0.1):
            for dense in (True, False):
                Lf = SoftTargetCrossEntropyLoss(eps)
                pl, pg, pc = Lf.loss_and_grad(xg, tg if dense else labg)
                cl, cg, _ = Lf.loss_and_grad(x.to(BF16).float(), t if dense else lab)
                torch.cuda.synchronize()
                grad = torch.zeros(N, C, dtype=BF16, device="cuda")
                loss, cor = ctypes.c_double(), ctypes.c_long()
                rc = L.dcnn_c_soft_loss(P(xg.data_ptr()), P(tg.data_ptr()) if dense else None,
                                        None if dense else P(labg.data_ptr()), P(grad.data_ptr()), ctypes.c_int(N),
                                        ctypes.c_int(C), ctypes.c_float(eps), ctypes.c_float(1.0), ctypes.byref(loss),
                                        ctypes.byref(cor))
                assert rc == 0, L.dcnn_c_last_error().decode()
                assert np.float32(loss.value) == np.float32(pl.item()) and cor.value == int(pc.item())
                assert torch.equal(grad, pg)
                assert abs(loss.value - float(cl)) < 1e-4 * max(1, abs(float(cl)))
                assert ((grad.float().cpu() - cg).norm() / cg.norm()).item() < 1e-2


@pytest.mark.gpu
def test_cpp_train_graph_with_a_dense_target_replays_the_eager_bits(parity, tmp_path):
    args = ["train", MODEL, "3", "6"]
    tail = ["--device", "GPU", "--mix"]
    e = _lines(_run([parity, *args, "snap/e", *tail], tmp_path).stdout)
    g = _lines(_run([parity, *args, "snap/g", *tail, "--graph"], tmp_path).stdout)
    assert len(e["losses"]) == 3 and all(np.isfinite(float(v)) for v in e["losses"])
    assert e["losses"] == g["losses"], (e["losses"], g["losses"])
    assert (tmp_path / "snap" / "e.bin").read_bytes() == (tmp_path / "snap" / "g.bin").read_bytes()


@pytest.mark.gpu
def test_cpp_train_graph_refuses_labels_after_a_dense_capture(parity, tmp_path):
    r = _run([parity, "train", MODEL, "3", "6", "snap/s", "--device", "GPU", "--mix", "--graph", "--switch-to-labels"],
             tmp_path, ok=False)
    assert r.returncode == 1 and "batch shape changed after capture" in r.stdout, r.stdout[-2000:]
    # eagerly the same sequence is fine: a loss takes either kind of target
    _run([parity, "train", MODEL, "3", "6", "snap/s", "--device", "GPU", "--mix", "--switch-to-labels"], tmp_path)
