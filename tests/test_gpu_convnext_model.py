"""ConvNeXt at the model level on the GPU: teacher-forced bf16 layers of a small ConvNeXt against the
bf16-emulated CPU backend (the method, wrapper and bounds of tests/test_gpu_dwconv_model.py, the
wrapper extended to LayerNorm, LayerScale and the GELU activation), the residual scale tail
(x + gamma F(x) in the LayerScale's store, dF + dS in the depthwise data gradient's store), hipGraph
replay of convnext_pico_cifar10, the fp32 compute dtype, and the conv geometries the ConvNeXt zoo
relies on (patchify stems, 2x2 / stride-2 transitions, the 1x1 pair of a block) against F.conv2d /
torch.nn.grad with tests/test_gpu_kernels.py's bounds."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CL = torch.channels_last


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def small_net():
    """input 3x16x16, stem 2x2 s2 -> 16 channels, one block, downsample -> 32, one block, head.
    Layer scale 0.5, not the zoo's 1e-6: the branch must weigh in the block's output."""
    from dcnn_amd.nn import SequentialBuilder
    return (SequentialBuilder("convnext_small").input([3, 16, 16])
            .conv2d(16, 2, 2, 2, 2, 0, 0, True, "stem_conv").layernorm(1e-6, True, "stem_ln")
            .convnext_block(16, 0.5, "block1")
            .convnext_downsample(32, "down2")
            .convnext_block(32, 0.5, "block2")
            .avgpool2d(4, 4, 1, 1, 0, 0, "avgpool").layernorm(1e-6, True, "head_ln").flatten("flatten")
            .dense(10, True, "fc").build())


def bf16_emulate(model):
    """tests/test_gpu_dwconv_model.py's wrapper, extended to LayerNorm, LayerScale and
    Activation("gelu"): parameters and every wrapped layer's input and output (forward and
    backward) rounded to bf16 on the CPU."""
    from dcnn_amd.nn.layers import (Activation, BatchNorm, Conv2D, Dense, DepthwiseConv2D, LayerNorm, LayerScale,
                                    ResidualBlock)
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(p.bfloat16().float())

    def r(t):
        return None if t is None else t.bfloat16().float()

    def wrap(l):
        f, b = l.forward, l.backward
        l.forward = lambda x, mb=0, **kw: r(f(r(x), mb, **{k: (r(v) if torch.is_tensor(v) else v) for k, v in kw.items()}))
        l.backward = lambda g, mb=0, **kw: r(b(r(g), mb, **{k: (r(v) if torch.is_tensor(v) else v) for k, v in kw.items()}))

    def walk(ls):
        for l in ls:
            if isinstance(l, ResidualBlock):
                walk(l.sublayers())
            elif isinstance(l, (Conv2D, DepthwiseConv2D, Dense, BatchNorm, LayerNorm, LayerScale)):
                wrap(l)
            elif isinstance(l, Activation) and l.activation_name == "gelu":
                wrap(l)
    walk(model.layers)
    return model


def _pair(seed=3, dtype=None):
    cpu = small_net()
    cpu.set_seed(seed)
    cpu.initialize()
    gpu = small_net()
    gpu.set_seed(seed)
    gpu.set_device("GPU:0")
    if dtype is not None:
        gpu.set_compute_dtype(dtype)
    gpu.initialize()
    for a, b in zip(cpu.parameters(), gpu.parameters()):
        assert torch.equal(a, b.cpu())
    return cpu, gpu


def test_convnext_layers_teacher_forced():
    from dcnn_amd.nn import LossFactory
    torch.manual_seed(0)
    B = 8
    x = torch.randn(B, 3, 16, 16)
    y = torch.randint(0, 10, (B,))
    cpu, gpu = _pair()
    assert [b._scale_tail for b in gpu.layers if b.type() == "residual_block"] == [True, True]
    bf16_emulate(cpu)
    gpu.load_parameters([p.clone() for p in cpu.parameters()])
    acts = [x]
    for l in cpu.layers:
        acts.append(l.forward(acts[-1]))
    _, g, _ = LossFactory.create("softmax_crossentropy").loss_and_grad(acts[-1], y)
    grads = [None] * len(cpu.layers)
    for i in range(len(cpu.layers) - 1, -1, -1):
        grads[i] = g
        g = cpu.layers[i].backward(g)
    cpu.clear_gradients()
    gpu.clear_gradients()
    for i, (lc, lg) in enumerate(zip(cpu.layers, gpu.layers)):
        lc.forward(acts[i])
        dxc = lc.backward(grads[i])
        out = lg.forward(acts[i].cuda())
        dxg = lg.backward(grads[i].cuda())
        e = rel(out, acts[i + 1])
        print(f"{lg.name}: fwd {e:.2e}", end="")
        assert e < 0.01, (lg.name, e)
        if dxc is not None and dxg is not None:
            e = rel(dxg, dxc)
            print(f" dx {e:.2e}", end="")
            assert e < 0.06, (lg.name, e)
        gc = [a.reshape(-1) for a in lc.gradients()]
        gg = [b.float().cpu().reshape(-1) for b in lg.gradients()]
        if gc:
            scale = max(a.norm().item() for a in gc)
            for j, (a, b) in enumerate(zip(gc, gg)):
                e = (a - b).norm().item() / max(a.norm().item(), 0.05 * scale)
                print(f" g{j} {e:.2e}", end="")
                assert e < 0.06, (lg.name, j, e)
        print()


def test_scale_tail_runs_without_a_separate_add():
    """The block's forward has one lscale_fwd carrying the residual, its backward a depthwise data
    gradient carrying the shortcut gradient; the result matches the CPU backend's plain path."""
    from dcnn_amd.nn.layers.residual import fuse_kinds
    from dcnn_amd.ops import hip
    from dcnn_amd.ops._ext import kernels
    torch.manual_seed(4)
    cpu, gpu = _pair(seed=6)
    with torch.no_grad():
        for p in cpu.parameters():
            p.copy_(p.bfloat16().float())
    gpu.load_parameters([p.clone() for p in cpu.parameters()])
    bc, bg = cpu.layers[2], gpu.layers[2]
    K = kernels()
    kinds = fuse_kinds(bg.main_path)
    assert kinds[-1] == K.FK_LSCALE
    assert K.plan_residual_fusions(kinds, [], True, True) == K.RF_SCALE_TAIL
    assert K.plan_residual_fusions(kinds, [], True, False) == 0  # a relu block keeps the plain path
    assert bg._scale_tail and not bg._fused and not bc._scale_tail
    x = torch.randn(8, 16, 8, 8).bfloat16().float()
    yc = bc.forward(x)
    with hip.record_convs() as calls:
        yg = bg.forward(x.cuda())
    ls = [c for c in calls if c["op"] == "lscale_fwd"]
    assert len(ls) == 1 and ls[0]["residual"] is True
    assert [c["op"] for c in calls if c["op"] in ("ln_fwd", "dw_fwd")] == ["dw_fwd", "ln_fwd"]
    assert rel(yg, yc) < 0.01, rel(yg, yc)
    dy = torch.randn_like(yc).bfloat16().float()
    dxc = bc.backward(dy)
    with hip.record_convs() as calls:
        dxg = bg.backward(dy.cuda())
    dg = [c for c in calls if c["op"] == "dw_dgrad"]
    assert len(dg) == 1 and dg[0]["residual"] is True
    assert [c["op"] for c in calls if c["op"] in ("lscale_bwd", "ln_bwd")] == ["lscale_bwd", "ln_bwd"]
    assert rel(dxg, dxc) < 0.06, rel(dxg, dxc)


def _convnext(seed=5):
    from dcnn_amd.models import create_model
    from dcnn_amd.nn import AdamW, LossFactory
    m = create_model("convnext_pico_cifar10")
    m.set_seed(seed)
    m.set_device("GPU:0")
    m.initialize()
    m.set_first_layer_input_grad(False)
    opt = AdamW(1e-3)
    opt.attach(m)
    return m, opt, LossFactory.create("softmax_crossentropy")


def test_convnext_graph_replay_matches_eager():
    from dcnn_amd.runtime.step import TrainStep
    torch.manual_seed(1)
    xs = [torch.randn(8, 3, 32, 32, device="cuda") for _ in range(2)]
    ys = [torch.randint(0, 10, (8,), device="cuda") for _ in range(2)]
    order = [0, 1, 0, 1, 0, 1]
    m, opt, lf = _convnext()
    st = TrainStep(m, lf, opt, use_graph=False)
    eager = []
    for i in order:
        st(xs[i], ys[i])
        eager.append(float(st.last_loss.item()))
    m2, opt2, lf2 = _convnext()
    st2 = TrainStep(m2, lf2, opt2, use_graph=True)
    graph = []
    for i in order:
        st2(xs[i], ys[i])
        graph.append(float(st2.last_loss.item()))
    assert st2.graphs is not None and opt2.t == opt.t
    assert all(v == v for v in eager)
    assert eager == graph, (eager, graph)
    assert torch.equal(m2.arena.data, m.arena.data)


def test_fp32_compute_dtype_matches_cpu():
    torch.manual_seed(0)
    cpu, gpu = _pair(seed=1, dtype=torch.float32)
    assert gpu.compute_dtype == torch.float32
    x = torch.randn(8, 3, 16, 16)
    yc = cpu.forward(x)
    yg = gpu.forward(x.cuda())
    err = rel(yg, yc)
    print(f"fp32 logits rel err {err:.2e}")
    assert err < 1e-4, err


def bf(t):
    return t.to(torch.bfloat16).float()


# N, Ci, H, W, Co, k, s, p
GEOMETRY = [
    (2, 3, 8, 8, 16, 4, 4, 0),    # ConvNeXt-T's patchify stem
    (2, 3, 8, 8, 16, 2, 2, 0),    # the CIFAR stem
    (2, 16, 4, 4, 32, 2, 2, 0),   # a stage transition
    (2, 96, 4, 4, 384, 1, 1, 0),  # a block's 1x1 pair
    (2, 384, 4, 4, 96, 1, 1, 0),
]


@pytest.mark.parametrize("case", GEOMETRY, ids=lambda c: "n{}c{}_{}x{}_o{}_k{}s{}p{}".format(*c))
def test_convnext_conv_geometry(case):
    """(i) forward (with bias), data gradient and weight gradient on the routes these shapes take."""
    from dcnn_amd.ops import hip
    N, Ci, H, W, Co, k, s, p = case
    torch.manual_seed(0)
    x = torch.randn(N, Ci, H, W)
    w = torch.randn(Co, Ci, k, k) / math.sqrt(Ci * k * k)
    b = torch.randn(Co)
    xb, wb = bf(x), bf(w)
    y_ref = F.conv2d(xb, wb, b, s, p)
    xg = x.cuda().to(torch.bfloat16).contiguous(memory_format=CL)
    wg = w.cuda().to(torch.bfloat16).contiguous(memory_format=CL)
    y, _ = hip.conv2d_fwd(xg, wg, b.cuda(), (s, s), (p, p))
    assert y.shape == y_ref.shape
    assert rel(y, y_ref) < 1e-2, rel(y, y_ref)
    dy = torch.randn_like(y_ref)
    dyb = bf(dy)
    dyg = dy.cuda().to(torch.bfloat16).contiguous(memory_format=CL)
    dx = hip.conv2d_dgrad(dyg, hip.conv_weight_t(wg), x.shape, (s, s), (p, p))
    dx_ref = torch.nn.grad.conv2d_input(x.shape, wb, dyb, s, p)
    assert rel(dx, dx_ref) < 1e-2, rel(dx, dx_ref)
    gw = torch.ones(Co, Ci, k, k, device="cuda").contiguous(memory_format=CL)
    gb = torch.ones(Co, device="cuda")
    hip.conv2d_wgrad(dyg, xg, w.shape, (s, s), (p, p), gw, gb)
    dw_ref = torch.nn.grad.conv2d_weight(xb, w.shape, dyb, s, p) + 1
    assert rel(gw, dw_ref) < 1e-2, rel(gw, dw_ref)
    assert rel(gb, dyb.sum((0, 2, 3)) + 1) < 1e-2
