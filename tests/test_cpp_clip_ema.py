"""Gradient clipping and the weight EMA in the C++ host API (csrc/host: Optimizer::set_max_grad_norm /
set_ema_decay / swap_ema / last_grad_norm, ParamArena::ema, TrainGraph, gpu_ops / cpu_ops grad_sumsq /
adam_tail / sgd_tail / ema_swap and the dcnn_c_* C ABI over them), through ctypes on libdcnn.so and
through examples/cpp/host_api_parity's ``train ... --clip-ema`` mode, like tests/test_cpp_drop_path.py.
The reference is the float64 formula of tests/test_clip_ema_cpu.py, or the Python front end."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from test_clip_ema_cpu import B1, B2, DECAY, EPS, LR, MOM, TOL, WD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dcnn_amd", "bin")
LIB = os.path.join(ROOT, "dcnn_amd", "libdcnn.so")
MODEL = "convnext_two_block"
P = ctypes.c_void_p
SIZES = [1, 3, 64, 4099, 4160, 2 ** 20 + 64]
CLIP = 0.25


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
    for name in ("grad_sumsq", "adam_tail", "sgd_tail", "ema_swap"):
        getattr(L, f"dcnn_c_{name}").restype = ctypes.c_int
        getattr(L, f"dcnn_c_{name}_host").restype = ctypes.c_int
    return L


def _ok(L, rc):
    assert rc == 0, L.dcnn_c_last_error().decode()


def _p(t):
    return P(t.data_ptr()) if t is not None else None


def _hp(*v):
    return (ctypes.c_float * len(v))(*v)


def _randn(n, seed, scale=1.0):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale


def _adam_ref(p, g, m, v, bc1, bc2, wd, decoupled, coef):
    g = g * coef
    m = B1 * m + (1 - B1) * g
    v = B2 * v + (1 - B2) * g * g
    upd = LR * (m / bc1) / ((v / bc2).sqrt() + EPS)
    if decoupled:
        p = p - wd * LR * p
    else:
        upd = upd + wd * LR * p
    return p - upd


def _check_entries(L, dev, n):
    """the four entry points on device `dev` ("cpu": the _host functions) at size n, one step each"""
    host = dev == "cpu"
    to = lambda t: t.to(dev)  # noqa: E731
    sync = (lambda: None) if host else torch.cuda.synchronize
    g = to(_randn(n, n, 3.0))
    want = float((g.double() ** 2).sum())
    mx = float(np.float32(0.3 * want ** 0.5))  # a bound under the norm at every n: the clip is active
    if host:
        s = ctypes.c_double(0.0)
        _ok(L, L.dcnn_c_grad_sumsq_host(_p(g), ctypes.c_long(n), ctypes.byref(s)))
        assert s.value == pytest.approx(want, rel=1e-12)
        coef_v = min(1.0, mx / (want ** 0.5 + 1e-6))
        coef_h = ctypes.c_double(coef_v)
        coef_arg = ctypes.byref(coef_h)
    else:
        out = torch.full((4,), -1.0, device=dev)
        sync()
        _ok(L, L.dcnn_c_grad_sumsq(_p(g), ctypes.c_long(n), ctypes.c_float(mx), _p(out)))
        norm = want ** 0.5
        ref = torch.tensor([want, norm, min(1.0, mx / (norm + 1e-6)), mx], dtype=torch.float64)
        assert torch.allclose(out.cpu().double(), ref, rtol=1e-5, atol=0)
        from dcnn_amd.ops import hip
        mine = torch.empty(4, device=dev)
        hip.grad_sumsq(g, mx, mine)
        sync()
        assert torch.equal(out, mine)  # the Python front end launches the same kernel: the same bits
        coef_v = float(out[2].item())
        coef_arg = P(out.data_ptr() + 8)
    p, m, e = _randn(n, 1), _randn(n, 3, 0.1), _randn(n, 5)
    v = _randn(n, 4, 0.1).abs()
    nodecay = (torch.rand((n + 63) // 64, generator=torch.Generator().manual_seed(6)) < 0.5).to(torch.uint8)
    wd = torch.where(nodecay.repeat_interleave(64)[:n].bool(), 0.0, WD).double()
    bc1, bc2 = 1 - B1 ** 3, 1 - B2 ** 3
    hp = _hp(LR, B1, B2, EPS, bc1, bc2, WD)
    for decoupled in (1, 0):
        pp, mm, vv, ee, nd = to(p.clone()), to(m.clone()), to(v.clone()), to(e.clone()), to(nodecay)
        sync()
        if host:
            _ok(L, L.dcnn_c_adam_tail_host(_p(pp), _p(g), _p(mm), _p(vv), ctypes.c_long(n), hp, decoupled, _p(nd),
                                           coef_arg, _p(ee), ctypes.c_float(DECAY)))
        else:
            _ok(L, L.dcnn_c_adam_tail(_p(pp), _p(g), _p(mm), _p(vv), None, ctypes.c_long(n), hp, decoupled, _p(nd),
                                      coef_arg, _p(ee), ctypes.c_float(DECAY)))
        rp = _adam_ref(p.double(), g.cpu().double(), m.double(), v.double(), bc1, bc2, wd, decoupled, coef_v)
        assert torch.allclose(pp.cpu(), rp.float(), **TOL)
        assert torch.allclose(ee.cpu(), (DECAY * e.double() + (1 - DECAY) * rp).float(), **TOL)
        unclipped = _adam_ref(p.double(), g.cpu().double(), m.double(), v.double(), bc1, bc2, wd, decoupled, 1.0)
        assert coef_v < 1 and not torch.allclose(pp.cpu(), unclipped.float(), **TOL)
    # SGD with momentum, then every optional input absent
    pp, vv, ee = to(p.clone()), to(m.clone()), to(e.clone())
    sync()
    hs = _hp(LR, MOM)
    if host:
        _ok(L, L.dcnn_c_sgd_tail_host(_p(pp), _p(g), _p(vv), ctypes.c_long(n), hs, coef_arg, _p(ee), ctypes.c_float(DECAY)))
    else:
        _ok(L, L.dcnn_c_sgd_tail(_p(pp), _p(g), _p(vv), None, ctypes.c_long(n), hs, coef_arg, _p(ee), ctypes.c_float(DECAY)))
    rv = MOM * m.double() - LR * g.cpu().double() * coef_v
    rp = p.double() + rv
    assert torch.allclose(pp.cpu(), rp.float(), **TOL) and torch.allclose(vv.cpu(), rv.float(), **TOL)
    assert torch.allclose(ee.cpu(), (DECAY * e.double() + (1 - DECAY) * rp).float(), **TOL)
    pp = to(p.clone())
    sync()
    if host:
        _ok(L, L.dcnn_c_sgd_tail_host(_p(pp), _p(g), None, ctypes.c_long(n), hs, None, None, ctypes.c_float(0.0)))
    else:
        _ok(L, L.dcnn_c_sgd_tail(_p(pp), _p(g), None, None, ctypes.c_long(n), hs, None, None, ctypes.c_float(0.0)))
    assert torch.allclose(pp.cpu(), (p.double() - LR * g.cpu().double()).float(), **TOL)
    # ema_swap: once exchanges, twice restores every bit
    a, b = to(_randn(n, 8)), to(_randn(n, 9))
    a0, b0 = a.clone(), b.clone()
    sync()
    for want_a, want_b in ((b0, a0), (a0, b0)):
        if host:
            _ok(L, L.dcnn_c_ema_swap_host(_p(a), _p(b), ctypes.c_long(n)))
        else:
            _ok(L, L.dcnn_c_ema_swap(_p(a), _p(b), None, ctypes.c_long(n)))
        assert torch.equal(a, want_a) and torch.equal(b, want_b)


@pytest.mark.parametrize("n", [1, 3, 64, 4099, 70001])
def test_c_abi_host_entries(parity, n):
    _check_entries(_lib(), "cpu", n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_c_abi_device_entries(parity, n):
    _check_entries(_lib(), "cuda", n)


def _python_run(tmp_path, name, steps, device=None):
    """the Python front end on host_api_parity's initial model and batches: AdamW, wd 0.1, the decay
    exclusion, max_grad_norm CLIP, ema_decay 0.9"""
    from dcnn_amd.nn import AdamW, LossFactory
    from dcnn_amd.nn.sequential import Sequential, load_tensor
    m = Sequential.from_file(str(tmp_path / "snap" / f"{name}.init"))
    if device is not None:
        m.set_device(device)
    m.set_training(True)
    opt = AdamW(1e-3, weight_decay=0.1, no_decay_norm_bias=True, max_grad_norm=CLIP, ema_decay=DECAY)
    opt.attach(m)
    lf = LossFactory.create("softmax_crossentropy")
    coefs = []
    for i in range(steps):
        with open(tmp_path / "snap" / f"{name}.x{i}.bin", "rb") as f:
            x = load_tensor(f)
        with open(tmp_path / "snap" / f"{name}.y{i}.bin", "rb") as f:
            y = load_tensor(f).reshape(-1).long()
        m.clear_gradients()
        _, grad, _ = lf.loss_and_grad(m.forward(x), y)
        m.backward(grad)
        opt.update()
        coefs.append(float(opt.grad_norm_device[2]))
    return m, opt, coefs


def test_cpp_train_graph_matches_python_front_end(parity, tmp_path):
    """Three TrainGraph steps of the two-block ConvNeXt model with both switches on (CPU backend:
    TrainGraph runs its step eagerly there) from host_api_parity's own initial weights and batches: the
    trained weights, the EMA weights and the last gradient norm equal the Python front end's."""
    from dcnn_amd.nn.sequential import Sequential
    (tmp_path / "snap").mkdir()
    out = _run([parity, "train", MODEL, "3", "6", "snap/c", "--adamw-no-decay", "--clip-ema", str(CLIP), "--graph"],
               tmp_path, timeout=300)
    assert len(out["losses"]) == 3 and all(np.isfinite(float(v)) for v in out["losses"])
    cpp = Sequential.from_file(str(tmp_path / "snap" / "c"))
    cpp_ema = Sequential.from_file(str(tmp_path / "snap" / "c.ema"))
    m, opt, coefs = _python_run(tmp_path, "c", 3)
    assert min(coefs) < 1.0, coefs  # the clip was active
    assert float(out["grad_norm"][0]) == pytest.approx(opt.last_grad_norm(), rel=1e-5)
    for k, (a, b) in enumerate(zip(cpp.parameters(), m.parameters())):
        assert torch.allclose(a, b, **TOL), k
    ema = [m.arena._view(opt.ema[0], i) for i in range(len(m.parameters()))]
    for k, (a, b) in enumerate(zip(cpp_ema.parameters(), ema)):
        assert torch.allclose(a, b, **TOL), k
    assert not all(torch.allclose(a, b, **TOL) for a, b in zip(cpp_ema.parameters(), cpp.parameters()))
    # and not the run with both switches off
    _run([parity, "train", MODEL, "3", "6", "snap/off", "--adamw-no-decay"], tmp_path, timeout=300)
    off = Sequential.from_file(str(tmp_path / "snap" / "off"))
    assert not all(torch.allclose(a, b, **TOL) for a, b in zip(cpp.parameters(), off.parameters()))


@pytest.mark.gpu
def test_cpp_train_graph_replay_matches_eager_gpu(parity, tmp_path):
    """The same run on the C++ GPU backend: the captured TrainGraph (norm reduction and tail kernel
    inside the graph, the EMA rolled back after the warm-up steps) leaves the bytes of the eager steps
    in the weights and in the EMA."""
    args = ["train", MODEL, "3", "6"]
    tail = ["--device", "GPU", "--adamw-no-decay", "--clip-ema", str(CLIP)]
    e = _run([parity, *args, "snap/e", *tail], tmp_path, timeout=300)
    g = _run([parity, *args, "snap/g", *tail, "--graph"], tmp_path, timeout=300)
    assert len(e["losses"]) == 3 and all(np.isfinite(float(v)) for v in e["losses"])
    assert e["losses"] == g["losses"] and e["grad_norm"] == g["grad_norm"]
    snap = tmp_path / "snap"
    assert (snap / "e.bin").read_bytes() == (snap / "g.bin").read_bytes()
    assert (snap / "e.ema.bin").read_bytes() == (snap / "g.ema.bin").read_bytes()
    assert (snap / "e.ema.bin").read_bytes() != (snap / "e.bin").read_bytes()
