"""LAMB and LARS in the C++ host API (csrc/host: dcnn::LAMB / dcnn::LARS, ParamArena::segments, TrainGraph,
gpu_ops / cpu_ops lamb / lars and the dcnn_c_* C ABI over them), through ctypes on libdcnn.so and through
examples/cpp/host_api_parity's ``train ... --opt lamb|lars`` mode, like tests/test_cpp_clip_ema.py. The
reference is the float64 formula of tests/test_gpu_lamb_lars.py over the same four arenas (one segment of
64; the seven slices; 1100 segments of 64; one segment of 2**20 + 64), or the Python front end.

On the GPU both front ends compute in bf16, and a layer-wise step is as sensitive to the sign of a
noise-level gradient as Adam's: there the comparison with the Python front end uses the bf16 tolerances
of tests/test_cpp_host_blocks.py::test_cpp_train_resnet18_gpu_vs_cpu (losses to 5e-2, the third to
1.5e-1), trust ratios (ratios of norms over whole parameters) to 5e-2, and asks that the trained
weights moved the same way (cosine of the whole update above 0.9). The tight comparison (TOL) is the
CPU backend's; captured against eager on the GPU is bit for bit."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from test_clip_ema_cpu import TOL
from test_gpu_lamb_lars import (ARENAS, B1, B2, BC1, BC2, DECAY, EPS, LARS_EPS, LR, MOM, RTOL, TC, WD, layout,
                                reference, state_of)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dcnn_amd", "bin")
LIB = os.path.join(ROOT, "dcnn_amd", "libdcnn.so")
MODEL = "convnext_two_block"
P = ctypes.c_void_p


@pytest.fixture(scope="module")
def parity():
    exe = os.path.join(BIN, "host_api_parity")
    if not (os.path.exists(exe) and os.path.exists(LIB)):
        from dcnn_amd import _build
        _build.build_host()
    return exe


def _run(cmd, cwd, timeout=600):
    r = subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:]
    return {l.split()[0]: l.split()[1:] for l in r.stdout.splitlines() if l.split()}


def _lib():
    L = ctypes.CDLL(LIB)
    L.dcnn_c_last_error.restype = ctypes.c_char_p
    for name in ("optim_segments", "lamb_step", "lars_step", "lamb_step_host", "lars_step_host"):
        getattr(L, f"dcnn_c_{name}").restype = ctypes.c_int
    return L


def _ok(L, rc):
    assert rc == 0, L.dcnn_c_last_error().decode()


def _p(t):
    return P(t.data_ptr()) if t is not None else None


def _tables(L, name):
    """the tables of arena ``name`` through dcnn_c_optim_segments: a size query, then the rows"""
    offs, counts, total, flags = layout(name)
    k = len(counts)
    c_off, c_cnt = (ctypes.c_long * k)(*offs), (ctypes.c_long * k)(*counts)
    c_flag = (ctypes.c_ubyte * k)(*[int(f) for f in flags])
    nch, cover = ctypes.c_int(-1), ctypes.c_long(-1)
    _ok(L, L.dcnn_c_optim_segments(c_off, c_cnt, c_flag, k, 1, ctypes.c_long(total), None, 0, None,
                                   ctypes.byref(nch), ctypes.byref(cover)))
    assert cover.value == total and nch.value == sum((n + 4095) // 4096 for n in counts)
    chunks = torch.zeros(nch.value, 3, dtype=torch.int32)
    segs = torch.zeros(k, 4, dtype=torch.int32)
    _ok(L, L.dcnn_c_optim_segments(c_off, c_cnt, c_flag, k, 1, ctypes.c_long(total), _p(chunks), nch.value, _p(segs),
                                   ctypes.byref(nch), ctypes.byref(cover)))
    from dcnn_amd.nn.params import SegmentTables
    mine = SegmentTables.from_slices(offs, list(counts), flags, True, total, "cpu")  # the Python front end's
    assert torch.equal(chunks, mine.chunks) and torch.equal(segs, mine.segs)
    assert L.dcnn_c_optim_segments(c_off, c_cnt, c_flag, k, 1, ctypes.c_long(total - 64), None, 0, None,
                                   ctypes.byref(nch), ctypes.byref(cover)) != 0
    assert b"ends at element" in L.dcnn_c_last_error()
    return chunks, segs, total


def _hp(*v):
    return (ctypes.c_double * len(v))(*v)


def _check_entries(L, dev, name, kind):
    """one step of ``kind`` on arena ``name`` through the C ABI on ``dev`` ("cpu": the _host functions),
    with the coefficient and the EMA, then with every optional input absent"""
    host = dev == "cpu"
    sync = (lambda: None) if host else torch.cuda.synchronize
    chunks, segs, total = _tables(L, name)
    ns, nc = segs.shape[0], chunks.shape[0]
    n = ctypes.c_long(total)
    for full in (True, False):
        b = {k: x.clone().to(dev) for k, x in state_of(name).items()}
        out = torch.full((3 * ns,), -1.0, dtype=torch.float64 if host else torch.float32, device=dev)
        coef_v = 0.37 if full else None
        ema = b["ema"] if full else None
        decay = ctypes.c_float(DECAY if full else 0.0)
        hp = (_hp(LR, B1, B2, EPS, BC1, BC2, WD) if kind == "lamb" else _hp(LR, MOM, WD, TC, LARS_EPS))
        if host:
            cf = ctypes.c_double(0.37)
            coef = ctypes.byref(cf) if full else None
            tab = (_p(chunks), nc, _p(segs), ns, _p(out))
            if kind == "lamb":
                _ok(L, L.dcnn_c_lamb_step_host(_p(b["p"]), _p(b["g"]), _p(b["m"]), _p(b["v"]), n, hp, coef, _p(ema), decay,
                                               *tab))
            else:
                _ok(L, L.dcnn_c_lars_step_host(_p(b["p"]), _p(b["g"]), _p(b["vel"]), n, hp, coef, _p(ema), decay, *tab))
        else:
            cdev = torch.tensor([0.37], device=dev) if full else None
            dch, dsg = chunks.to(dev), segs.to(dev)
            part = torch.zeros(max(2 * nc, 1), device=dev)  # a partial pair per chunk
            sync()
            tab = (_p(dch), nc, _p(dsg), ns, n, _p(part), _p(out))
            if kind == "lamb":
                _ok(L, L.dcnn_c_lamb_step(_p(b["p"]), _p(b["g"]), _p(b["m"]), _p(b["v"]), None, n, hp, None, _p(cdev),
                                          _p(ema), decay, *tab))
            else:
                _ok(L, L.dcnn_c_lars_step(_p(b["p"]), _p(b["g"]), _p(b["vel"]), None, n, hp, None, _p(cdev), _p(ema),
                                          decay, *tab))
            sync()
        want = reference(kind, name, coef_v, full)
        got = out.cpu().double()
        assert torch.allclose(got[:ns], torch.tensor(want["trust"], dtype=torch.float64), rtol=RTOL, atol=0)
        assert torch.allclose(got[ns:].reshape(ns, 2), torch.tensor(want["sums"], dtype=torch.float64), rtol=RTOL, atol=0)
        for k in ["p"] + (["m", "v"] if kind == "lamb" else ["vel"]) + (["ema"] if full else []):
            assert torch.allclose(b[k].cpu().double(), want[k], **TOL), (k, full)
        assert any(abs(t - 1.0) > 0.05 for t in want["trust"])


@pytest.mark.parametrize("name", list(ARENAS))
@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_c_abi_host_entries(parity, kind, name):
    _check_entries(_lib(), "cpu", name, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ARENAS))
@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_c_abi_device_entries(parity, kind, name):
    _check_entries(_lib(), "cuda", name, kind)


def test_c_abi_refuses_a_table_past_the_buffer(parity):
    L = _lib()
    chunks, segs, total = _tables(L, "seven")
    z = torch.zeros(total - 64)
    out = torch.zeros(3 * segs.shape[0], dtype=torch.float64)
    rc = L.dcnn_c_lars_step_host(_p(z), _p(z.clone()), None, ctypes.c_long(total - 64), _hp(0.1, 0.0, 0.0, 1e-3, 1e-8),
                                 None, None, ctypes.c_float(0.0), _p(chunks), chunks.shape[0], _p(segs), segs.shape[0],
                                 _p(out))
    assert rc != 0 and b"does not fit" in L.dcnn_c_last_error()


def _python_opt(kind):
    """host_api_parity's --opt settings in the Python front end"""
    from dcnn_amd.nn import LAMB, LARS
    if kind == "lamb":
        return LAMB(1e-3, 0.9, 0.999, 1e-6, 0.1, no_decay_norm_bias=True)
    return LARS(0.5, 0.9, 0.01, 0.02, 1e-8, no_decay_norm_bias=True)


def _python_run(tmp_path, name, steps, kind, device=None):
    from dcnn_amd.nn import LossFactory
    from dcnn_amd.nn.sequential import Sequential, load_tensor
    m = Sequential.from_file(str(tmp_path / "snap" / f"{name}.init"))
    if device is not None:
        m.set_device(device)
    m.set_training(True)
    opt = _python_opt(kind)
    opt.attach(m)
    lf = LossFactory.create("softmax_crossentropy")
    losses = []
    for i in range(steps):
        with open(tmp_path / "snap" / f"{name}.x{i}.bin", "rb") as f:
            x = load_tensor(f)
        with open(tmp_path / "snap" / f"{name}.y{i}.bin", "rb") as f:
            y = load_tensor(f).reshape(-1).long()
        if device is not None:
            x, y = x.cuda(), y.cuda()
        m.clear_gradients()
        loss, grad, _ = lf.loss_and_grad(m.forward(x), y)
        m.backward(grad)
        opt.update()
        losses.append(float(loss))
    return m, opt, losses


@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_cpp_train_graph_matches_python_front_end(parity, tmp_path, kind):
    """Three TrainGraph steps of the two-block ConvNeXt model (CPU backend: TrainGraph runs its step
    eagerly there, the optimizer on its per-parameter path) from host_api_parity's own initial weights and
    batches: losses, trained weights and the last step's trust ratios equal the Python front end's."""
    from dcnn_amd.nn.sequential import Sequential
    (tmp_path / "snap").mkdir()
    out = _run([parity, "train", MODEL, "3", "6", "snap/c", "--opt", kind, "--graph"], tmp_path, timeout=300)
    m, opt, losses = _python_run(tmp_path, "c", 3, kind)
    assert [float(v) for v in out["losses"]] == pytest.approx(losses, rel=1e-5)
    trust = opt.last_trust_ratios()
    assert [float(v) for v in out["trust"]] == pytest.approx(trust, rel=1e-5)
    flags = m.no_decay_flags()
    assert all(t == 1.0 for t, f in zip(trust, flags) if f) and any(abs(t - 1.0) > 0.05 for t in trust)
    cpp = Sequential.from_file(str(tmp_path / "snap" / "c"))
    for k, (a, b) in enumerate(zip(cpp.parameters(), m.parameters())):
        assert torch.allclose(a, b, **TOL), k
    # and not the plain Adam run
    _run([parity, "train", MODEL, "3", "6", "snap/off"], tmp_path, timeout=300)
    off = Sequential.from_file(str(tmp_path / "snap" / "off"))
    assert not all(torch.allclose(a, b, **TOL) for a, b in zip(cpp.parameters(), off.parameters()))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_cpp_gpu_captured_matches_eager_and_the_python_front_end(parity, tmp_path, kind):
    """The same run on the C++ GPU backend: the captured TrainGraph (both launches of the step and the
    static tables inside the graph, the state rolled back after the warm-up steps) leaves the bytes of the
    eager steps; against the Python front end on GPU:0, bf16 tolerances (module docstring)."""
    from dcnn_amd.nn.sequential import Sequential
    (tmp_path / "snap").mkdir()
    args = ["train", MODEL, "3", "6"]
    tail = ["--device", "GPU", "--opt", kind]
    e = _run([parity, *args, "snap/e", *tail], tmp_path, timeout=300)
    g = _run([parity, *args, "snap/g", *tail, "--graph"], tmp_path, timeout=300)
    assert len(e["losses"]) == 3 and all(np.isfinite(float(v)) for v in e["losses"])
    assert e["losses"] == g["losses"] and e["trust"] == g["trust"]
    snap = tmp_path / "snap"
    assert (snap / "e.bin").read_bytes() == (snap / "g.bin").read_bytes()
    assert (snap / "e.bin").read_bytes() != (snap / "e.init.bin").read_bytes()
    m, opt, losses = _python_run(tmp_path, "g", 3, kind, "GPU:0")
    torch.cuda.synchronize()
    got = [float(v) for v in g["losses"]]
    print(kind, "losses", got, losses)
    np.testing.assert_allclose(got[:2], losses[:2], rtol=5e-2)
    np.testing.assert_allclose(got[2], losses[2], rtol=1.5e-1)
    trust = opt.last_trust_ratios()
    print(kind, "trust", g["trust"], trust)
    np.testing.assert_allclose([float(v) for v in g["trust"]], trust, rtol=5e-2)
    init = Sequential.from_file(str(snap / "g.init"))
    cpp = Sequential.from_file(str(snap / "g"))
    da = torch.cat([(a - i).flatten() for a, i in zip(cpp.parameters(), init.parameters())]).double()
    db = torch.cat([(b.detach().cpu() - i).flatten() for b, i in zip(m.parameters(), init.parameters())]).double()
    cos = float((da * db).sum() / (da.norm() * db.norm()))
    print(kind, "update cosine", cos)
    assert cos > 0.9
