"""GroupedConv2D at the model level on the GPU: teacher-forced bf16 layers against the bf16-emulated
CPU backend (the method and bounds of tests/test_gpu_dwconv_model.py / tests/test_gpu_model.py), a
residual block whose main path starts with the grouped layer, hipGraph replay of ResNeXt-26 and the
fp32 compute dtype."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def small_net():
    """stem 32 -> ResNeXt block (32, 32, 64, G = 8, s1) -> ResNeXt block (64, 64, 128, G = 8, s2) -> head:
    grouped 3x3s of 4 and 8 channels per group, stride 1 and 2."""
    from dcnn_amd.nn import SequentialBuilder
    b = SequentialBuilder("gc_small").input([3, 16, 16])
    b.conv2d(32, 3, 3, 1, 1, 1, 1, False, "conv1").batchnorm(1e-5, 0.1, True, "bn1").activation("relu", "relu1")
    b.resnext_bottleneck_block(32, 32, 64, 8, 1, "block1").resnext_bottleneck_block(64, 64, 128, 8, 2, "block2")
    return b.avgpool2d(8, 8, 1, 1, 0, 0, "avgpool").flatten("flatten").dense(10, True, "fc").build()


def bf16_emulate(model):
    """tests/test_gpu_model.py's wrapper, extended to GroupedConv2D: parameters and every conv /
    dense / BatchNorm input and output (forward and backward) rounded to bf16 on the CPU."""
    from dcnn_amd.nn.layers import BatchNorm, Conv2D, Dense, GroupedConv2D, ResidualBlock
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
            elif isinstance(l, (Conv2D, GroupedConv2D, Dense, BatchNorm)):
                wrap(l)
    walk(model.layers)
    return model


def test_grouped_layers_teacher_forced_and_unfused():
    from dcnn_amd.nn import LossFactory
    from dcnn_amd.nn.layers import Activation, BatchNorm, GroupedConv2D, ResidualBlock
    from dcnn_amd.nn.layers.residual import fuse_kinds
    from dcnn_amd.ops import hip
    from dcnn_amd.ops._ext import kernels
    torch.manual_seed(0)
    B = 8
    x = torch.randn(B, 3, 16, 16)
    y = torch.randint(0, 10, (B,))
    cpu = small_net()
    cpu.set_seed(3)
    cpu.initialize()
    gpu = small_net()
    gpu.set_seed(3)
    gpu.set_device("GPU:0")
    gpu.initialize()
    for a, b in zip(cpu.parameters(), gpu.parameters()):
        assert torch.equal(a, b.cpu())
    # the planner sees the grouped layers as FK_OTHER: no statistics epilogue, no bnb role
    blocks = [l for l in gpu.layers if isinstance(l, ResidualBlock)]
    assert len(blocks) == 2
    for blk in blocks:
        kinds = fuse_kinds(blk.main_path)
        gi = [i for i, l in enumerate(blk.main_path) if isinstance(l, GroupedConv2D)]
        assert gi == [3] and kinds[3] == kernels().FK_OTHER and kinds[0] == kernels().FK_CONV
        assert not getattr(blk.main_path[3], "emit_bn_stats", False)
    for l in gpu.layers:
        if isinstance(l, BatchNorm):
            l.fuse_pool = None
    bf16_emulate(cpu)
    acts = [x]
    for l in cpu.layers:
        acts.append(l.forward(acts[-1]))
    _, g, _ = LossFactory.create("softmax_crossentropy").loss_and_grad(acts[-1], y)
    grads = [None] * len(cpu.layers)
    for i in range(len(cpu.layers) - 1, -1, -1):
        grads[i] = g
        g = cpu.layers[i].backward(g)
    cpu.clear_gradients()
    ran = []
    for i, (lc, lg) in enumerate(zip(cpu.layers, gpu.layers)):
        if isinstance(lg, Activation) and lg.passthrough:
            continue  # fused into the preceding BatchNorm
        nxt_relu = isinstance(lg, BatchNorm) and lg.fuse_relu
        lc.forward(acts[i])
        dxc = lc.backward(grads[i] * (acts[i + 1] > 0) if nxt_relu else grads[i])
        with hip.record_convs() as calls:
            out = lg.forward(acts[i].cuda())
            dxg = lg.backward(grads[i].cuda())
        ran += [c["op"] for c in calls if c["op"].startswith("gc_")]
        ref = torch.relu(acts[i + 1]) if nxt_relu else acts[i + 1]
        print(f"{lg.name}: fwd {rel(out, ref):.3e}" + (f" dx {rel(dxg, dxc):.3e}" if dxc is not None and dxg is not None
                                                       else ""))
        assert rel(out, ref) < 0.01, (lg.name, rel(out, ref))
        if dxc is not None and dxg is not None:
            assert rel(dxg, dxc) < 0.06, (lg.name, rel(dxg, dxc))
        gc = [a.reshape(-1) for a in lc.gradients()]
        gg = [b.float().cpu().reshape(-1) for b in lg.gradients()]
        if gc:
            scale = max(a.norm().item() for a in gc)
            for j, (a, b) in enumerate(zip(gc, gg)):
                e = (a - b).norm().item() / max(a.norm().item(), 0.05 * scale)
                assert e < 0.06, (lg.name, j, e)
    assert sorted(ran) == ["gc_dgrad"] * 2 + ["gc_fwd"] * 2 + ["gc_wgrad"] * 2  # the gconv.hip kernels ran


def _res_model():
    from dcnn_amd.nn import SequentialBuilder
    from dcnn_amd.nn.layers import LayerBuilder
    main = (LayerBuilder().input([32, 8, 8]).grouped_conv2d(32, 3, 3, 4, 1, 1, 1, 1, False, "gc")
            .batchnorm(1e-5, 0.1, True, "bn0").activation("relu", "relu0")
            .conv2d(32, 1, 1, 1, 1, 0, 0, False, "pw").batchnorm(1e-5, 0.1, True, "bn1").build())
    return SequentialBuilder("gc_res").input([32, 8, 8]).residual(main, [], "relu", "block").build()


def test_residual_block_starting_with_grouped():
    """Identity shortcut: the block's input gradient dF + dS comes out of the grouped dgrad's store
    (add_to -> residual) and equals the unfused sum dgrad(g) + dS."""
    from dcnn_amd.ops import hip
    torch.manual_seed(4)
    cpu = _res_model()
    cpu.set_seed(6)
    cpu.initialize()
    with torch.no_grad():
        for p in cpu.parameters():
            p.copy_(p.bfloat16().float())
    gpu = _res_model()
    gpu.set_seed(6)
    gpu.set_device("GPU:0")
    gpu.initialize()
    gpu.load_parameters([p.clone() for p in cpu.parameters()])
    cpu.set_first_layer_input_grad(True)
    gpu.set_first_layer_input_grad(True)
    x = torch.randn(8, 32, 8, 8).bfloat16().float()
    yc = cpu.forward(x)
    yg = gpu.forward(x.cuda())
    assert rel(yg, yc) < 0.02, rel(yg, yc)
    dy = torch.randn_like(yc).bfloat16().float()
    dxc = cpu.backward(dy)
    with hip.record_convs() as calls:
        dxg = gpu.backward(dy.cuda())
    dg = [c for c in calls if c["op"] == "gc_dgrad"]
    assert len(dg) == 1 and dg[0]["residual"] is True and dg[0]["groups"] == 4
    assert rel(dxg, dxc) < 0.06, rel(dxg, dxc)


def test_fused_add_to_equals_unfused_sum():
    """The dgrad the block above issues (residual = dS) against the plain dgrad + dS on the same
    operands. The fused store rounds F + s once; the unfused sum uses round(F): per element
    |fused - (round(F) + s)| <= 2^-8 |F + s| + 2^-8 |F| <= 2^-7 (|ref| + |plain|)."""
    from dcnn_amd.ops import hip
    CL = torch.channels_last
    torch.manual_seed(2)
    w = (torch.randn(32, 8, 3, 3, device="cuda") / 72 ** 0.5).bfloat16().contiguous(memory_format=CL)
    dy = torch.randn(8, 32, 8, 8, device="cuda").bfloat16().contiguous(memory_format=CL)
    s = torch.randn(8, 32, 8, 8, device="cuda").bfloat16().contiguous(memory_format=CL)
    fused = hip.gconv2d_dgrad(dy, w, (8, 32, 8, 8), (1, 1), (1, 1), 4, residual=s)
    plain = hip.gconv2d_dgrad(dy, w, (8, 32, 8, 8), (1, 1), (1, 1), 4).float()
    ref = plain + s.float()
    assert ((fused.float() - ref).abs() <= 2.0 ** -7 * (ref.abs() + plain.abs())).all()
    assert rel(fused, ref) < 5e-3


def _resnext(seed=5):
    from dcnn_amd.models import create_model
    from dcnn_amd.nn import Adam, LossFactory
    m = create_model("resnext26_32x4d_cifar10")
    m.set_seed(seed)
    m.set_device("GPU:0")
    m.initialize()
    m.set_first_layer_input_grad(False)
    opt = Adam(1e-3)
    opt.attach(m)
    return m, opt, LossFactory.create("softmax_crossentropy")


def test_resnext_graph_replay_matches_eager():
    from dcnn_amd.runtime.step import TrainStep
    torch.manual_seed(1)
    xs = [torch.randn(8, 3, 32, 32, device="cuda") for _ in range(2)]
    ys = [torch.randint(0, 10, (8,), device="cuda") for _ in range(2)]
    order = [0, 1, 0, 1, 0, 1]
    m, opt, lf = _resnext()
    st = TrainStep(m, lf, opt, use_graph=False)
    eager = []
    for i in order:
        st(xs[i], ys[i])
        eager.append(float(st.last_loss.item()))
    m2, opt2, lf2 = _resnext()
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
    cpu = small_net()
    cpu.set_seed(1)
    cpu.initialize()
    gpu = cpu.clone()
    gpu.set_device("GPU:0")
    gpu.set_compute_dtype(torch.float32)
    gpu.initialize()
    gpu.load_parameters([p.clone() for p in cpu.parameters()])
    assert gpu.compute_dtype == torch.float32
    x = torch.randn(8, 3, 16, 16)
    yc = cpu.forward(x)
    yg = gpu.forward(x.cuda())
    err = rel(yg, yc)
    print(f"fp32 logits rel err {err:.2e}")
    assert err < 1e-4, err
