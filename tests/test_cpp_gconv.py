"""Grouped convolution in the C++ host API (csrc/host: GroupedConv2D, gpu_ops / cpu_ops gconv_*, the
dcnn_c_gconv_* C ABI, ResNeXt in dcnn::create_model), driven through examples/cpp/host_api_parity
like tests/test_cpp_dwconv.py and checked against the Python front end and fp32 PyTorch."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dcnn_amd", "bin")
LIB = os.path.join(ROOT, "dcnn_amd", "libdcnn.so")
MODEL = "resnext26_32x4d_cifar10"
CL = torch.channels_last
BF16 = torch.bfloat16
P = ctypes.c_void_p


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


def _grouped(m):
    from dcnn_amd.nn import GroupedConv2D
    return [l.main_path[3] for l in m.layers if l.type() == "residual_block" and isinstance(l.main_path[3], GroupedConv2D)]


def test_cpp_and_python_cpu_gradients_identical(parity, tmp_path):
    """ResNeXt-26 on the CPU backend of both front ends: the same initial weights and batch give
    bit-identical parameter gradients (both run the native grouped kernels; covers layer order, the
    config keys and the (Co, Ci/G, KH, KW) parameter layout across the checkpoint)."""
    from dcnn_amd.nn import LossFactory
    from dcnn_amd.nn.sequential import Sequential, load_tensor
    from dcnn_amd.parallel.dp import DataParallel
    (tmp_path / "snap").mkdir()
    out = _lines(_run([parity, "grads", MODEL, "2", "g.bin", "snap/init"], tmp_path, timeout=300))
    with open(tmp_path / "g.bin", "rb") as f:
        gc = [load_tensor(f) for _ in out["params"]]
    m = Sequential.from_file(str(tmp_path / "snap" / "init"))
    gl = _grouped(m)
    assert len(gl) == 8 and all(l.groups == 32 for l in gl)
    assert [tuple(l.weights.shape) for l in gl] == [(c, c // 32, 3, 3) for c in (128, 128, 256, 256, 512, 512, 1024, 1024)]
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
    assert len(gp) == len(gc) == 89
    for k, (a, b) in enumerate(zip(gp, gc)):
        assert torch.equal(a.detach().reshape(b.shape), b), k


def test_python_checkpoint_runs_in_cpp(parity, tmp_path):
    from dcnn_amd.models import create_model
    from dcnn_amd.nn import SGD, LossFactory
    from dcnn_amd.nn.sequential import save_tensor
    m = create_model(MODEL)
    m.set_seed(4)
    m.initialize()
    opt = SGD(0.01)
    opt.attach(m)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 3, 32, 32, generator=g)
    y = torch.randint(0, 10, (2,), generator=g)
    out = m.forward(x)
    _, grad, _ = LossFactory.create("softmax_crossentropy").loss_and_grad(out, y)
    m.backward(grad)
    opt.update()  # moves the weights and the BN running statistics away from their init
    m.set_training(False)
    with torch.no_grad():
        ref = m.forward(x).reshape(2, -1).double().numpy()
    m.save_to_file(str(tmp_path / "py" / "m"))
    with open(tmp_path / "x.bin", "wb") as f:
        save_tensor(f, x)
    got = _lines(_run([parity, "forward", "py/m", "x.bin"], tmp_path))
    assert int(got["params"][0]) == sum(p.numel() for p in m.parameters())
    logits = np.array([float(v) for v in got["logits"]]).reshape(2, -1)
    rel = np.linalg.norm(logits - ref) / np.linalg.norm(ref)
    assert rel < 1e-4, rel


def _segments(out):
    rows = []
    for line in out.splitlines():
        if line.startswith("segment "):
            f = line.split()
            rows.append((f[3], float(f[5]), float(f[7]), float(f[9]), f[10], float(f[12]), float(f[14])))
    return rows


@pytest.mark.gpu
def test_cpp_gpu_segments_teacher_forced(parity, tmp_path):
    """Every segment of ResNeXt-26 on the C++ GPU backend against the CPU backend's fp32 step, fed the
    CPU input and output gradient. The grouped layers sit inside the residual-block segments, which
    stay within tests/test_cpp_host_blocks.py's bounds (fwd <= 2e-2, bwd and parameters <= 0.2,
    cosines >= 0.99)."""
    out = _run([parity, "blocks", MODEL, "16", "--device", "GPU"], tmp_path, timeout=600)
    rows = _segments(out)
    print("segments (name, fwd rel, bwd rel, param rel, worst param, bwd cosine, param cosine):")
    for row in rows:
        print(row)
    blocks = [r for r in rows if r[0].startswith("layer")]
    assert len(blocks) == 8, out[-2000:]
    bad = [r for r in rows if r[1] > 2e-2 or r[2] > 0.2 or r[3] > 0.2 or r[5] < 0.99 or r[6] < 0.99]
    assert not bad, bad


@pytest.mark.gpu
def test_cpp_train_graph_replay_matches_eager(parity, tmp_path):
    """The grouped layer inside the captured TrainGraph step: graph replay and eager steps give the
    same losses and the same bytes in the saved weights."""
    args = ["train", MODEL, "4", "8"]
    e = _lines(_run([parity, *args, "snap/e", "--device", "GPU"], tmp_path, timeout=300))
    g = _lines(_run([parity, *args, "snap/g", "--device", "GPU", "--graph"], tmp_path, timeout=300))
    assert len(e["losses"]) == 4 and all(np.isfinite(float(v)) for v in e["losses"])
    assert e["losses"] == g["losses"], (e["losses"], g["losses"])
    assert (tmp_path / "snap" / "e.bin").read_bytes() == (tmp_path / "snap" / "g.bin").read_bytes()


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _excess(y, ref, A, K):
    """tests/test_gpu_gconv.py's per-element bound 2^-7 |ref| + 2 K 2^-24 A (<= 1 passes)."""
    err = (y.float().cpu() - ref).abs()
    bound = ref.abs() * 2.0 ** -7 + 2.0 * K * 2.0 ** -24 * A
    zero = torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err))
    return torch.where(bound > 0, err / bound, zero).max().item()


# cases 2, 4, 5 and 9 of tests/test_gpu_gconv.py: (N, Ci, Co, G, H, W, stride), 3x3 pad 1
ABI_CASES = [(2, 32, 32, 8, 5, 7, 1), (2, 64, 64, 4, 9, 9, 2), (2, 64, 128, 2, 8, 8, 1), (2, 24, 24, 3, 8, 8, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("deferred", [0, 1], ids=["immediate", "deferred"])
@pytest.mark.parametrize("case", ABI_CASES, ids=["cig4", "s2", "cig32", "halfbundle"])
def test_c_abi_gconv_calls(parity, case, deferred):
    """dcnn_c_gconv_fwd / dgrad / wgrad against PyTorch fp32 with the bounds of tests/test_gpu_gconv.py."""
    L = ctypes.CDLL(LIB)
    L.dcnn_c_last_error.restype = ctypes.c_char_p
    for name in ("dcnn_c_gconv_fwd", "dcnn_c_gconv_dgrad", "dcnn_c_gconv_wgrad"):
        getattr(L, name).restype = ctypes.c_int
    N, Ci, Co, G, H, W, s = case
    Cig, Cog = Ci // G, Co // G
    g = torch.Generator().manual_seed(1234)
    bf = lambda t: t.to(BF16).float()  # noqa: E731
    x = bf(torch.randn(N, Ci, H, W, generator=g))
    w = bf(torch.randn(Co, Cig, 3, 3, generator=g) / (9 * Cig) ** 0.5)
    b = torch.randn(Co, generator=g)
    y_ref = F.conv2d(x, w, b, s, 1, groups=G)
    y_abs = F.conv2d(x.abs(), w.abs(), None, s, 1, groups=G)
    OH, OW = y_ref.shape[2:]
    dy, res = bf(torch.randn(y_ref.shape, generator=g)), bf(torch.randn(N, Ci, H, W, generator=g))
    dx_ref = torch.nn.grad.conv2d_input(x.shape, w, dy, s, 1, groups=G) + res
    dx_abs = torch.nn.grad.conv2d_input(x.shape, w.abs(), dy.abs(), s, 1, groups=G) + res.abs()
    dw_ref = torch.nn.grad.conv2d_weight(x, w.shape, dy, s, 1, groups=G)
    shape = (ctypes.c_int * 13)(N, Ci, H, W, Co, 3, 3, s, s, 1, 1, OH, OW)
    act = lambda t: t.cuda().to(BF16).contiguous(memory_format=CL)  # noqa: E731
    xg, dyg, rg, wg, bg = act(x), act(dy), act(res), act(w), b.cuda()
    y = torch.empty(N, Co, OH, OW, device="cuda", dtype=BF16).contiguous(memory_format=CL)
    dx = torch.empty(N, Ci, H, W, device="cuda", dtype=BF16).contiguous(memory_format=CL)
    gw = torch.ones(Co, Cig, 3, 3, device="cuda").contiguous(memory_format=CL)
    gb = torch.ones(Co, device="cuda")
    torch.cuda.synchronize()

    def ok(rc):
        assert rc == 0, L.dcnn_c_last_error().decode()

    cg = ctypes.c_int(G)
    ok(L.dcnn_c_gconv_fwd(P(xg.data_ptr()), P(wg.data_ptr()), P(bg.data_ptr()), P(y.data_ptr()), shape, cg))
    ok(L.dcnn_c_gconv_dgrad(P(dyg.data_ptr()), P(wg.data_ptr()), P(dx.data_ptr()), shape, cg, P(rg.data_ptr())))
    ok(L.dcnn_c_gconv_wgrad(P(dyg.data_ptr()), P(xg.data_ptr()), P(gw.data_ptr()), P(gb.data_ptr()), shape, cg,
                            ctypes.c_int(deferred)))
    torch.cuda.synchronize()
    assert _rel(y, y_ref) < 1e-2 and _excess(y, y_ref, y_abs, Cig * 9) <= 1.0
    assert _rel(dx, dx_ref) < 1e-2 and _excess(dx, dx_ref, dx_abs, Cog * 9) <= 1.0
    assert _rel(gw, dw_ref + 1) < 1e-4 and _rel(gb, dy.sum((0, 2, 3)) + 1) < 1e-4
    # a shape outside the supported set is an error through the ABI, not a fallback
    assert L.dcnn_c_gconv_fwd(P(xg.data_ptr()), P(wg.data_ptr()), None, P(y.data_ptr()), shape, ctypes.c_int(5)) == -1
    assert "grouped conv" in L.dcnn_c_last_error().decode()
