"""ConvNeXt in the C++ host API (csrc/host: LayerNorm, LayerScale, GELU in Activation, gpu_ops /
cpu_ops layernorm_* / layer_scale_*, the dcnn_c_layernorm_* / dcnn_c_layer_scale_* C ABI, the scale
tail of ResidualBlock, ConvNeXt in dcnn::create_model), driven through examples/cpp/host_api_parity
like tests/test_cpp_dwconv.py and checked against the Python front end."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dcnn_amd", "bin")
LIB = os.path.join(ROOT, "dcnn_amd", "libdcnn.so")
MODEL = "convnext_pico_cifar10"
CL = torch.channels_last
BF16 = torch.bfloat16
P = ctypes.c_void_p
BLOCKS = [f"stage{s}_block{i}" for s, n in enumerate((2, 2, 6, 2), 1) for i in range(1, n + 1)]


@pytest.fixture(scope="module")
def parity():
    exe = os.path.join(BIN, "host_api_parity")
    if not (os.path.exists(exe) and os.path.exists(LIB) and torch.cuda.is_available()):
        from dcnn_amd import _build
        _build.build_host()
    return exe


def _run(cmd, cwd, timeout=600):
    r = subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:]
    return r.stdout


def _lines(out):
    d = {}
    for l in out.splitlines():
        parts = l.split()
        if parts:
            d[parts[0]] = parts[1:]
    return d


def _structure(m):
    from dcnn_amd.nn import LayerNorm, LayerScale
    blocks = [l for l in m.layers if l.type() == "residual_block"]
    assert [b.name for b in blocks] == BLOCKS
    for b in blocks:
        assert [l.name for l in b.main_path] == ["depthwise_conv2d_0", "layernorm_1", "conv2d_2", "activation_3",
                                                 "conv2d_4", "layer_scale_5"]
        assert isinstance(b.main_path[1], LayerNorm) and isinstance(b.main_path[5], LayerScale)
        assert b.main_path[3].activation_name == "gelu" and b.activation_type == "none" and not b.shortcut_path
    assert [l.name for l in m.layers if isinstance(l, LayerNorm)] == ["stem_ln", "down2_ln", "down3_ln", "down4_ln",
                                                                     "head_ln"]


def test_cpp_and_python_cpu_gradients_identical(parity, tmp_path):
    """ConvNeXt on the CPU backend of both front ends: the same initial weights and batch give
    bit-identical parameter gradients (both run the native LayerNorm / LayerScale / GELU kernels;
    covers layer order, names and the parameter layouts across the checkpoint)."""
    from dcnn_amd.models import create_model
    from dcnn_amd.nn import LossFactory
    from dcnn_amd.nn.sequential import Sequential, load_tensor
    from dcnn_amd.parallel.dp import DataParallel
    (tmp_path / "snap").mkdir()
    out = _lines(_run([parity, "grads", MODEL, "2", "g.bin", "snap/init"], tmp_path, timeout=300))
    with open(tmp_path / "g.bin", "rb") as f:
        gc = [load_tensor(f) for _ in out["params"]]
    m = Sequential.from_file(str(tmp_path / "snap" / "init"))
    _structure(m)
    ref = create_model(MODEL)
    assert [(l.type(), l.name) for l in m.layers] == [(l.type(), l.name) for l in ref.layers]
    for a, b in zip(m.layers, ref.layers):  # (C++ keeps epsilon / init_value as float)
        ca, cb = a.get_config().parameters, b.get_config().parameters
        if a.type() == "residual_block":
            ca, cb = ({k: v for k, v in c.items() if not k.endswith("_path")} for c in (ca, cb))
        assert ca.keys() == cb.keys(), a.name
        for k in ca:
            assert ca[k] == (pytest.approx(cb[k], rel=1e-6) if isinstance(cb[k], float) else cb[k]), (a.name, k)
    m.set_training(True)
    with open(tmp_path / "snap" / "init.x.bin", "rb") as f:
        x = load_tensor(f)
    with open(tmp_path / "snap" / "init.y.bin", "rb") as f:
        y = load_tensor(f).reshape(-1).long()
    dp = DataParallel(m, broadcast=False)
    m.clear_gradients()
    loss, grad, _ = LossFactory.create("softmax_crossentropy").loss_and_grad(dp.forward(x), y)
    assert abs(float(loss) - float(out["loss"][0])) < 1e-5
    dp.backward(grad, prescaled=True)
    gp = m.gradients()
    assert len(gp) == len(gc) == 128
    for k, (a, b) in enumerate(zip(gp, gc)):
        assert torch.equal(a.detach().reshape(b.shape), b), k


def _spread_layer_scale(m):
    """layer scale 1e-6 leaves the branches invisible in the logits: give them weight"""
    with torch.no_grad():
        for b in (l for l in m.layers if l.type() == "residual_block"):
            b.main_path[-1].parameters()[0].fill_(0.5)


def test_python_checkpoint_runs_in_cpp(parity, tmp_path):
    from dcnn_amd.models import create_model
    from dcnn_amd.nn import SGD, LossFactory
    from dcnn_amd.nn.sequential import save_tensor
    m = create_model(MODEL)
    m.set_seed(4)
    m.initialize()
    _spread_layer_scale(m)
    opt = SGD(0.01)
    opt.attach(m)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 3, 32, 32, generator=g)
    y = torch.randint(0, 10, (2,), generator=g)
    out = m.forward(x)
    _, grad, _ = LossFactory.create("softmax_crossentropy").loss_and_grad(out, y)
    m.backward(grad)
    opt.update()  # moves the weights (LayerNorm and LayerScale parameters too) away from their init
    m.set_training(False)
    with torch.no_grad():
        ref = m.forward(x).reshape(2, -1).double().numpy()
    m.save_to_file(str(tmp_path / "py" / "m"))
    with open(tmp_path / "x.bin", "wb") as f:
        save_tensor(f, x)
    got = _lines(_run([parity, "forward", "py/m", "x.bin"], tmp_path))
    assert int(got["params"][0]) == sum(p.numel() for p in m.parameters()) == 8535498
    logits = np.array([float(v) for v in got["logits"]]).reshape(2, -1)
    rel = np.linalg.norm(logits - ref) / np.linalg.norm(ref)
    assert rel < 1e-4, rel


def test_cpp_trained_model_loads_in_python(parity, tmp_path):
    from dcnn_amd.nn.sequential import Sequential, save_tensor
    out = _lines(_run([parity, "train", MODEL, "3", "4", "snap/cn"], tmp_path, timeout=300))
    losses = [float(v) for v in out["losses"]]
    assert len(losses) == 3 and all(np.isfinite(losses))
    m = Sequential.from_file(str(tmp_path / "snap" / "cn"))
    _structure(m)
    m.set_training(False)
    x = torch.randn(3, 3, 32, 32, generator=torch.Generator().manual_seed(1))
    with open(tmp_path / "x.bin", "wb") as f:
        save_tensor(f, x)
    got = _lines(_run([parity, "forward", "snap/cn", "x.bin"], tmp_path))
    with torch.no_grad():
        ref = m.forward(x).reshape(3, -1).double().numpy()
    cpp = np.array([float(v) for v in got["logits"]]).reshape(3, -1)
    assert np.linalg.norm(cpp - ref) / np.linalg.norm(ref) < 1e-4


def _segments(out):
    rows = []
    for line in out.splitlines():
        if line.startswith("segment "):
            f = line.split()
            rows.append((f[3], float(f[5]), float(f[7]), float(f[9]), f[10], float(f[12]), float(f[14])))
    return rows


@pytest.mark.gpu
def test_cpp_gpu_segments_teacher_forced(parity, tmp_path):
    """Every segment of ConvNeXt on the C++ GPU backend against the CPU backend's fp32 step, fed the
    CPU input and output gradient, within tests/test_cpp_dwconv.py's bounds: the single-layer
    segments (the LayerNorms among them) fwd < 2e-2, bwd and parameters < 6e-2, the blocks fwd
    <= 2e-2, bwd and parameters <= 0.2; cosines >= 0.99."""
    out = _run([parity, "blocks", MODEL, "16", "--device", "GPU"], tmp_path, timeout=600)
    rows = _segments(out)
    print("segments (name, fwd rel, bwd rel, param rel, worst param, bwd cosine, param cosine):")
    for row in rows:
        print(row)
    lns = [r for r in rows if r[0].endswith("_ln")]
    assert len(lns) == 5, out[-2000:]
    bad = [r for r in lns if r[1] >= 2e-2 or r[2] >= 6e-2 or r[3] >= 6e-2 or r[5] < 0.99 or r[6] < 0.99]
    assert not bad, bad
    rest = [r for r in rows if not r[0].endswith("_ln")]
    assert len([r for r in rest if r[0] in BLOCKS]) == 12
    bad = [r for r in rest if r[1] > 2e-2 or r[2] > 0.2 or r[3] > 0.2 or r[5] < 0.99 or r[6] < 0.99]
    assert not bad, bad


@pytest.mark.gpu
def test_cpp_train_graph_replay_matches_eager(parity, tmp_path):
    args = ["train", MODEL, "4", "8"]
    e = _lines(_run([parity, *args, "snap/e", "--device", "GPU"], tmp_path, timeout=300))
    g = _lines(_run([parity, *args, "snap/g", "--device", "GPU", "--graph"], tmp_path, timeout=300))
    assert len(e["losses"]) == 4 and all(np.isfinite(float(v)) for v in e["losses"])
    assert e["losses"] == g["losses"], (e["losses"], g["losses"])
    assert (tmp_path / "snap" / "e.bin").read_bytes() == (tmp_path / "snap" / "g.bin").read_bytes()


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(70, 96), (33, 768), (20011, 64)], ids=lambda c: f"{c[0]}x{c[1]}")
def test_c_abi_matches_python_front_end(parity, case):
    """dcnn_c_layernorm_* / dcnn_c_layer_scale_* on the same device tensors give the bits the Python
    front end gives (ops.hip.ln_* / lscale_*): the kernels are the same."""
    from dcnn_amd.ops import hip
    L = ctypes.CDLL(LIB)
    L.dcnn_c_last_error.restype = ctypes.c_char_p
    for name in ("dcnn_c_layernorm_fwd", "dcnn_c_layernorm_bwd", "dcnn_c_layer_scale_fwd", "dcnn_c_layer_scale_bwd"):
        getattr(L, name).restype = ctypes.c_int
    R, C = case
    g = torch.Generator().manual_seed(31)
    x, dy, res = (torch.randn(R, C, generator=g).to(BF16).cuda() for _ in range(3))
    gamma, beta = (1 + 0.5 * torch.randn(C, generator=g)).cuda(), torch.randn(C, generator=g).cuda()
    y, mean, rstd = hip.ln_fwd(x, gamma, beta, 1e-6)
    dg, db, dls = (torch.ones(C, device="cuda") for _ in range(3))
    dx = hip.ln_bwd(dy, x, gamma, mean, rstd, dg, db)
    ys = hip.lscale_fwd(x, gamma, res)
    dxs = hip.lscale_bwd(dy, x, gamma, dls)
    y2, dx2, ys2, dxs2 = (torch.empty_like(x) for _ in range(4))
    mean2, rstd2 = torch.empty_like(mean), torch.empty_like(rstd)
    dg2, db2, dls2 = (torch.ones(C, device="cuda") for _ in range(3))
    torch.cuda.synchronize()

    def ok(rc):
        assert rc == 0, L.dcnn_c_last_error().decode()

    p = lambda t: P(t.data_ptr())  # noqa: E731
    Rc, Cc = ctypes.c_long(R), ctypes.c_int(C)
    ok(L.dcnn_c_layernorm_fwd(p(x), p(y2), Rc, Cc, p(gamma), p(beta), ctypes.c_float(1e-6), p(mean2), p(rstd2)))
    ok(L.dcnn_c_layernorm_bwd(p(dy), p(x), p(dx2), Rc, Cc, p(gamma), p(mean2), p(rstd2), p(dg2), p(db2)))
    ok(L.dcnn_c_layer_scale_fwd(p(x), p(gamma), p(res), p(ys2), Rc, Cc))
    ok(L.dcnn_c_layer_scale_bwd(p(dy), p(x), p(gamma), p(dxs2), p(dls2), Rc, Cc))
    for a, b in ((y, y2), (mean, mean2), (rstd, rstd2), (dx, dx2), (dg, dg2), (db, db2), (ys, ys2), (dxs, dxs2),
                 (dls, dls2)):
        assert torch.equal(a, b)
    assert L.dcnn_c_layernorm_fwd(p(x), p(y2), Rc, ctypes.c_int(12), None, None, ctypes.c_float(1e-6), p(mean2),
                                  p(rstd2)) == -1
    assert "C 12" in L.dcnn_c_last_error().decode()
