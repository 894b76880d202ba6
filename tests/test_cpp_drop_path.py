"""DropPath and the weight-decay exclusion in the C++ host API (csrc/host: dcnn::DropPath, the drop
tail of ResidualBlock, Adam::set_no_decay_norm_bias, gpu_ops / cpu_ops drop_path_* /
layer_scale_drop_*, the dcnn_c_drop_path_* / dcnn_c_layer_scale_drop_* C ABI, drop_path_rate in
dcnn::create_model), driven through examples/cpp/host_api_parity like tests/test_cpp_convnext.py and
checked against the Python front end. The CPU model is host_api_parity's "convnext_two_block": two
ConvNeXt blocks (C = 16, 8x8 map) with DropPath at rate 0.5 and explicit seeds, so both front ends
draw the same masks."""
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
SEEDS = [101, (1 << 40) + 7]
CL = torch.channels_last
BF16 = torch.bfloat16
P = ctypes.c_void_p
TOL = dict(atol=1e-6, rtol=1e-5)  # tests/test_training_components.py::test_optimizer_update_rules


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
    return r.stdout


def _lines(out):
    d = {}
    for l in out.splitlines():
        parts = l.split()
        if parts:
            d[parts[0]] = parts[1:]
    return d


def _drop_paths(m):
    return [b.main_path[-1] for b in m.layers if b.type() == "residual_block"]


def _load_init(tmp_path):
    from dcnn_amd.nn.sequential import Sequential, load_tensor
    m = Sequential.from_file(str(tmp_path / "snap" / "init"))
    with open(tmp_path / "snap" / "init.x.bin", "rb") as f:
        x = load_tensor(f)
    with open(tmp_path / "snap" / "init.y.bin", "rb") as f:
        y = load_tensor(f).reshape(-1).long()
    dps = _drop_paths(m)
    assert [(d.type(), d.name, d.drop_rate, d.explicit_seed) for d in dps] == \
        [("drop_path", "drop_path_6", 0.5, s) for s in SEEDS]
    return m, x, y


def test_cpp_and_python_cpu_gradients_identical(parity, tmp_path):
    """The two-block model on the CPU backend of both front ends: the same initial weights, batch and
    explicit DropPath seeds give the same masks and bit-identical parameter gradients."""
    from dcnn_amd.nn import LossFactory
    from dcnn_amd.nn.sequential import load_tensor
    from dcnn_amd.ops import cpu
    (tmp_path / "snap").mkdir()
    out = _lines(_run([parity, "grads", MODEL, "6", "g.bin", "snap/init"], tmp_path, timeout=300))
    with open(tmp_path / "g.bin", "rb") as f:
        gc = [load_tensor(f) for _ in out["params"]]
    m, x, y = _load_init(tmp_path)
    m.set_training(True)
    m.clear_gradients()
    loss, grad, _ = LossFactory.create("softmax_crossentropy").loss_and_grad(m.forward(x), y)
    assert abs(float(loss) - float(out["loss"][0])) < 1e-5
    m.backward(grad)
    both = False
    for d, s in zip(_drop_paths(m), SEEDS):
        mk = d.last_mask()
        assert torch.equal(mk, cpu.drop_path_mask(s, 1, 6, 0.5))
        both = both or ((mk == 0).any().item() and (mk != 0).any().item())
    assert both
    gp = m.gradients()
    assert len(gp) == len(gc) == 26
    for k, (a, b) in enumerate(zip(gp, gc)):
        assert torch.equal(a.detach().reshape(b.shape), b), k


def test_python_checkpoint_runs_in_cpp(parity, tmp_path):
    """A Python checkpoint with drop_path layers (explicit seed and derived) loads in C++; in eval mode
    the DropPath is the identity and the logits agree."""
    from dcnn_amd.nn import SequentialBuilder
    from dcnn_amd.nn.sequential import save_tensor
    m = (SequentialBuilder("py_dp").input([3, 16, 16])
         .conv2d(16, 2, 2, 2, 2, 0, 0, True, "stem_conv").layernorm(1e-6, True, "stem_ln")
         .convnext_block(16, 0.5, "block1", drop_path=0.25, drop_path_seed=(1 << 40) + 3)
         .convnext_block(16, 0.5, "block2", drop_path=0.5)
         .drop_path(0.125, "dp_top")
         .avgpool2d(8, 8, 1, 1, 0, 0, "avgpool").layernorm(1e-6, True, "head_ln").flatten("flatten")
         .dense(10, True, "fc").build())
    m.set_seed(4)
    m.initialize()
    m.set_training(False)
    x = torch.randn(3, 3, 16, 16, generator=torch.Generator().manual_seed(9))
    with torch.no_grad():
        ref = m.forward(x).reshape(3, -1).double().numpy()
    m.save_to_file(str(tmp_path / "py" / "m"))
    with open(tmp_path / "x.bin", "wb") as f:
        save_tensor(f, x)
    got = _lines(_run([parity, "forward", "py/m", "x.bin"], tmp_path))
    assert int(got["params"][0]) == sum(p.numel() for p in m.parameters())
    logits = np.array([float(v) for v in got["logits"]]).reshape(3, -1)
    rel = np.linalg.norm(logits - ref) / np.linalg.norm(ref)
    assert rel < 1e-4, rel


def test_cpp_trained_model_loads_in_python(parity, tmp_path):
    from dcnn_amd.nn.sequential import Sequential, save_tensor
    out = _lines(_run([parity, "train", MODEL, "3", "4", "snap/cn", "--adamw-no-decay"], tmp_path, timeout=300))
    losses = [float(v) for v in out["losses"]]
    assert len(losses) == 3 and all(np.isfinite(losses))
    m = Sequential.from_file(str(tmp_path / "snap" / "cn"))
    assert [d.explicit_seed for d in _drop_paths(m)] == SEEDS
    m.set_training(False)
    x = torch.randn(3, 3, 16, 16, generator=torch.Generator().manual_seed(1))
    with open(tmp_path / "x.bin", "wb") as f:
        save_tensor(f, x)
    got = _lines(_run([parity, "forward", "snap/cn", "x.bin"], tmp_path))
    with torch.no_grad():
        ref = m.forward(x).reshape(3, -1).double().numpy()
    cpp = np.array([float(v) for v in got["logits"]]).reshape(3, -1)
    assert np.linalg.norm(cpp - ref) / np.linalg.norm(ref) < 1e-4


def test_decay_exclusion_step_matches_between_front_ends(parity, tmp_path):
    """One AdamW step (wd 0.1, biases / norm affines / layer scales excluded) from the same weights on
    the same batch, with the same DropPath masks: the C++ parameters equal the Python ones within the
    fused-Adam tolerance, and differ from a step that decays everything."""
    from dcnn_amd.nn import AdamW, LossFactory
    from dcnn_amd.nn.sequential import Sequential
    (tmp_path / "snap").mkdir()
    _run([parity, "grads", MODEL, "6", "g.bin", "snap/init"], tmp_path, timeout=300)
    _run([parity, "train", MODEL, "1", "6", "snap/step", "--adamw-no-decay"], tmp_path, timeout=300)
    cpp = Sequential.from_file(str(tmp_path / "snap" / "step"))

    def step(no_decay):
        m, x, y = _load_init(tmp_path)
        m.set_training(True)
        opt = AdamW(1e-3, weight_decay=0.1, no_decay_norm_bias=no_decay)
        opt.attach(m)
        m.clear_gradients()
        _, grad, _ = LossFactory.create("softmax_crossentropy").loss_and_grad(m.forward(x), y)
        m.backward(grad)
        opt.update()
        return m

    py, full = step(True), step(False)
    flags = py.no_decay_flags()
    assert any(flags) and not all(flags)
    for k, (a, b) in enumerate(zip(cpp.parameters(), py.parameters())):
        assert torch.allclose(a, b, **TOL), k
    differs = [not torch.allclose(a, b, **TOL) for a, b in zip(cpp.parameters(), full.parameters())]
    assert any(d for d, f in zip(differs, flags) if f)


def test_cpp_zoo_drop_path_rate(parity, tmp_path):
    """dcnn::create_model(name, drop_path_rate): the layers, names and rates of the Python zoo."""
    from dcnn_amd.models import create_model
    from dcnn_amd.nn.sequential import Sequential
    (tmp_path / "snap").mkdir()
    _run([parity, "grads", "convnext_pico_cifar10", "2", "g.bin", "snap/z", "--drop-path", "0.1",
          "--seed-drop-path"], tmp_path, timeout=300)
    m = Sequential.from_file(str(tmp_path / "snap" / "z"))
    ref = create_model("convnext_pico_cifar10", drop_path_rate=0.1)
    names = lambda mm: [(l.type(), l.name, [(s.type(), s.name) for s in l.main_path] if l.type() == "residual_block"  # noqa: E731
                         else None) for l in mm.layers]
    assert names(m) == names(ref)
    blocks = [l for l in m.layers if l.type() == "residual_block"]
    dps = [(k, b.main_path[-1]) for k, b in enumerate(blocks) if b.main_path[-1].type() == "drop_path"]
    assert [k for k, _ in dps] == list(range(1, 12))
    assert [d.drop_rate for _, d in dps] == pytest.approx([0.1 * i / 11 for i in range(1, 12)], rel=1e-6)
    assert [d.explicit_seed for _, d in dps] == [1000 + k for k, _ in dps]


# ------------------------------------------------------------------------------------------- GPU
def _lib():
    L = ctypes.CDLL(LIB)
    L.dcnn_c_last_error.restype = ctypes.c_char_p
    for name in ("dcnn_c_drop_path_mask", "dcnn_c_drop_path_mask_host", "dcnn_c_drop_path_scale",
                 "dcnn_c_layer_scale_drop_fwd", "dcnn_c_layer_scale_drop_bwd"):
        getattr(L, name).restype = ctypes.c_int
    return L


def test_c_abi_host_mask_equals_the_native_module(parity):
    """dcnn_c_drop_path_mask_host: the C ABI's CPU mask is the native module's, bit for bit."""
    from dcnn_amd.ops import cpu
    L = _lib()
    for seed in (1, (1 << 40) + 3):
        for draw in (1, 2, 1000):
            for n in (1, 3, 4, 5, 257):
                for p in (0.1, 0.5):
                    buf = torch.full((n,), -1.0)
                    rc = L.dcnn_c_drop_path_mask_host(P(buf.data_ptr()), ctypes.c_long(n), ctypes.c_float(p),
                                                      ctypes.c_uint64(seed), ctypes.c_uint64(draw))
                    assert rc == 0, L.dcnn_c_last_error().decode()
                    assert torch.equal(buf, cpu.drop_path_mask(seed, draw, n, p))
    assert L.dcnn_c_drop_path_mask_host(P(buf.data_ptr()), ctypes.c_long(1), ctypes.c_float(1.0), ctypes.c_uint64(1),
                                        ctypes.c_uint64(1)) == -1


@pytest.mark.gpu
def test_c_abi_mask_equals_python_kernels(parity):
    from dcnn_amd.ops import cpu
    from dcnn_amd.ops._ext import kernels
    L = _lib()
    for seed in (1, (1 << 40) + 3):
        for draw in (1, 2, 1000):
            for n in (1, 3, 4, 5, 257):
                for p in (0.1, 0.5):
                    buf = torch.full((n,), -1.0, device="cuda")
                    torch.cuda.synchronize()
                    rc = L.dcnn_c_drop_path_mask(P(buf.data_ptr()), ctypes.c_int(n), ctypes.c_float(p),
                                                 ctypes.c_uint64(seed), ctypes.c_uint64(draw))
                    assert rc == 0, L.dcnn_c_last_error().decode()
                    ref = torch.tensor(kernels().drop_path_mask(seed, draw, n, p))
                    assert torch.equal(buf.cpu(), ref) and torch.equal(ref, cpu.drop_path_mask(seed, draw, n, p))


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(6, 16, 4, 4), (5, 96, 3, 3), (2, 2048, 1, 1)], ids=lambda c: "x".join(map(str, c)))
def test_c_abi_kernels_equal_python_front_end(parity, case):
    """dcnn_c_drop_path_scale / dcnn_c_layer_scale_drop_* on the same device tensors give the bits of
    ops.hip.drop_path_scale / lscale_drop_*: the kernels are the same."""
    from dcnn_amd.ops import cpu, hip
    L = _lib()
    N, C, H, W = case
    g = torch.Generator().manual_seed(31)
    x, dy, res = (torch.randn(case, generator=g).to(BF16).cuda().contiguous(memory_format=CL) for _ in range(3))
    gamma = (1 + 0.5 * torch.randn(C, generator=g)).cuda()
    seed = next(s for s in range(1, 64) if 0 < int((cpu.drop_path_mask(s, 1, N, 0.5) != 0).sum()) < N)
    mask = cpu.drop_path_mask(seed, 1, N, 0.5).cuda()
    ys, dxs = hip.drop_path_scale(x, mask), hip.drop_path_scale(dy, mask)
    yr = hip.drop_path_scale(x, mask, res)
    yt = hip.lscale_drop_fwd(x, gamma, mask, res)
    dg = torch.ones(C, device="cuda")
    dxt = hip.lscale_drop_bwd(dy, x, gamma, mask, dg)
    ys2, dxs2, yr2, yt2, dxt2 = (torch.empty_like(x) for _ in range(5))
    dg2 = torch.ones(C, device="cuda")
    torch.cuda.synchronize()

    def ok(rc):
        assert rc == 0, L.dcnn_c_last_error().decode()

    p = lambda t: P(t.data_ptr())  # noqa: E731
    Nc, row = ctypes.c_long(N), ctypes.c_long(C * H * W)
    R, Cc, rps = ctypes.c_long(N * H * W), ctypes.c_int(C), ctypes.c_long(H * W)
    ok(L.dcnn_c_drop_path_scale(p(x), p(mask), None, p(ys2), Nc, row))
    ok(L.dcnn_c_drop_path_scale(p(dy), p(mask), None, p(dxs2), Nc, row))
    ok(L.dcnn_c_drop_path_scale(p(x), p(mask), p(res), p(yr2), Nc, row))
    ok(L.dcnn_c_layer_scale_drop_fwd(p(x), p(gamma), p(mask), p(res), p(yt2), R, Cc, rps))
    ok(L.dcnn_c_layer_scale_drop_bwd(p(dy), p(x), p(gamma), p(mask), p(dxt2), p(dg2), R, Cc, rps))
    for a, b in ((ys, ys2), (dxs, dxs2), (yr, yr2), (yt, yt2), (dxt, dxt2), (dg, dg2)):
        assert torch.equal(a, b)
    assert L.dcnn_c_layer_scale_drop_fwd(p(x), p(gamma), p(mask), p(res), p(yt2), R, ctypes.c_int(12), rps) == -1
    assert "C 12" in L.dcnn_c_last_error().decode()


@pytest.mark.gpu
def test_cpp_train_graph_replay_matches_eager(parity, tmp_path):
    """Three AdamW steps (decay exclusion on) of the two-block model with DropPath on the C++ GPU
    backend: the captured TrainGraph's replays draw the masks the eager steps draw, so the losses and
    the saved parameters are identical."""
    args = ["train", MODEL, "3", "6"]
    tail = ["--device", "GPU", "--adamw-no-decay"]
    e = _lines(_run([parity, *args, "snap/e", *tail], tmp_path, timeout=300))
    g = _lines(_run([parity, *args, "snap/g", *tail, "--graph"], tmp_path, timeout=300))
    assert len(e["losses"]) == 3 and all(np.isfinite(float(v)) for v in e["losses"])
    assert e["losses"] == g["losses"], (e["losses"], g["losses"])
    assert (tmp_path / "snap" / "e.bin").read_bytes() == (tmp_path / "snap" / "g.bin").read_bytes()
