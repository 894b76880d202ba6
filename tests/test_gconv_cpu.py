"""Grouped convolution on the native CPU backend and the GroupedConv2D layer plumbing (factory,
builders, checkpoints, the ResNeXt block and zoo models). Oracle: F.conv2d(groups=G) and autograd."""
import json

import pytest
import torch
import torch.nn.functional as F

# the first twelve kernel cases of tests/test_gpu_gconv.py:
# (N, Ci, Co, G, H, W, (KH, KW), (SH, SW), (PH, PW))
CASES = [
    (1, 8, 16, 2, 1, 1, (3, 3), (1, 1), (1, 1)),
    (2, 32, 32, 8, 5, 7, (3, 3), (1, 1), (1, 1)),
    (2, 64, 64, 8, 16, 16, (3, 3), (1, 1), (1, 1)),
    (2, 64, 64, 4, 9, 9, (3, 3), (2, 2), (1, 1)),
    (2, 64, 128, 2, 8, 8, (3, 3), (1, 1), (1, 1)),
    (1, 128, 128, 2, 6, 6, (3, 3), (1, 1), (1, 1)),
    (2, 256, 256, 2, 4, 4, (3, 3), (1, 1), (1, 1)),
    (2, 48, 96, 3, 7, 5, (3, 3), (2, 2), (1, 1)),
    (2, 24, 24, 3, 8, 8, (3, 3), (1, 1), (1, 1)),
    (2, 64, 32, 4, 8, 8, (1, 1), (1, 1), (0, 0)),
    (2, 32, 32, 4, 10, 6, (5, 5), (1, 1), (2, 2)),
    (2, 16, 32, 2, 10, 6, (1, 3), (1, 2), (0, 1)),
]
_ids = [f"n{c[0]}c{c[1]}o{c[2]}g{c[3]}_{c[4]}x{c[5]}_k{c[6][0]}x{c[6][1]}_s{c[7][0]}{c[7][1]}_p{c[8][0]}{c[8][1]}"
        for c in CASES]


def rel(a, r):
    return ((a - r).norm() / (r.norm() + 1e-300)).item()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_native_grouped_matches_torch(case, dtype):
    from dcnn_amd.ops import cpu
    N, Ci, Co, G, H, W, (KH, KW), st, pd = case
    Cig = Ci // G
    tol = 1e-5 if dtype == torch.float32 else 1e-12
    g = torch.Generator().manual_seed(1234)
    x = torch.randn(N, Ci, H, W, dtype=dtype, generator=g, requires_grad=True)
    w = (torch.randn(Co, Cig, KH, KW, dtype=dtype, generator=g) / (Cig * KH * KW) ** 0.5).requires_grad_()
    b = torch.randn(Co, dtype=dtype, generator=g, requires_grad=True)
    ref = F.conv2d(x, w, b, st, pd, groups=G)
    dy = torch.randn(ref.shape, dtype=dtype, generator=g)
    ref.backward(dy)

    y = cpu.grouped_conv2d_fwd(x.detach(), w.detach(), b.detach(), st, pd, G)
    assert y.dtype == dtype and rel(y, ref.detach()) < tol
    y0 = cpu.grouped_conv2d_fwd(x.detach(), w.detach(), None, st, pd, G)
    assert rel(y0, F.conv2d(x, w, None, st, pd, groups=G).detach()) < tol
    # accumulation into non-zero gradients
    gw = torch.full((Co, Cig, KH, KW), 0.5, dtype=dtype)
    gb = torch.full((Co,), -2.0, dtype=dtype)
    dx = cpu.grouped_conv2d_bwd(x.detach(), w.detach(), dy, st, pd, G, gw, gb)
    assert rel(dx, x.grad) < tol and rel(gw, w.grad + 0.5) < tol and rel(gb, b.grad - 2.0) < tol
    # need_dx=False: parameter gradients only
    gw2 = torch.zeros(Co, Cig, KH, KW, dtype=dtype)
    assert cpu.grouped_conv2d_bwd(x.detach(), w.detach(), dy, st, pd, G, gw2, None, need_dx=False) is None
    assert rel(gw2, w.grad) < tol


def test_native_grouped_rejects_bad_groups():
    from dcnn_amd.ops import cpu
    x, w = torch.zeros(1, 12, 4, 4), torch.zeros(8, 3, 3, 3)
    with pytest.raises(ValueError, match="groups 5"):
        cpu.grouped_conv2d_fwd(x, w, None, (1, 1), (1, 1), 5)
    with pytest.raises(ValueError, match="groups 2"):  # weights have 12 / 4 input channels per filter
        cpu.grouped_conv2d_fwd(x, w, None, (1, 1), (1, 1), 2)


def test_layer_config_roundtrip_factory_and_builders():
    from dcnn_amd.nn import GroupedConv2D, LayerFactory, Sequential, SequentialBuilder
    from dcnn_amd.nn.layers import Conv2D, DepthwiseConv2D, LayerBuilder, create_layer
    assert "grouped_conv2d" in LayerFactory.available_types()
    l = GroupedConv2D(24, 48, 5, 3, 3, 2, 1, 2, 1, False, "gx")
    assert not isinstance(l, (Conv2D, DepthwiseConv2D)) and l.type() == "grouped_conv2d"
    cfg = l.get_config()
    assert cfg.parameters == dict(in_channels=24, out_channels=48, kernel_h=5, kernel_w=3, groups=3, stride_h=2,
                                  stride_w=1, pad_h=2, pad_w=1, use_bias=False)
    again = create_layer("grouped_conv2d", cfg)
    assert isinstance(again, GroupedConv2D) and again.get_config().parameters == cfg.parameters
    assert again.name == "gx"
    assert l.compute_output_shape([4, 24, 11, 9]) == [4, 48, 6, 9]
    # a dense conv's FLOPs divided by G
    assert l.forward_flops([4, 24, 11, 9]) == 2 * 48 * (24 // 3) * 15 * 4 * 6 * 9
    assert l.forward_flops([4, 24, 11, 9]) * 3 == Conv2D(24, 48, 5, 3, 2, 1, 2, 1, False).forward_flops([4, 24, 11, 9])
    assert l.backward_flops([4, 24, 11, 9]) == 2 * l.forward_flops([4, 24, 11, 9])
    assert GroupedConv2D(8, 16, 3, 3, 2).forward_flops([1, 8, 4, 4]) == 2 * 16 * 4 * 9 * 4 + 16 * 4
    assert [tuple(s.shape) for s in GroupedConv2D(8, 16, 3, 3, 2).param_specs()] == [(16, 4, 3, 3), (16, 1, 1, 1)]
    # builders infer the input channel count from the running shape
    lb = LayerBuilder().input([12, 8, 8]).grouped_conv2d(24, 3, 3, 3, 2, 2, 1, 1, True, "a").build()
    assert (lb[0].in_channels, lb[0].out_channels, lb[0].groups) == (12, 24, 3) and lb[0].use_bias
    m = (SequentialBuilder("s").input([3, 8, 8]).conv2d(16, 3, 3, 1, 1, 1, 1)
         .grouped_conv2d(32, 3, 3, 4, 2, 2, 1, 1).build())
    assert m.layers[1].in_channels == 16 and m.compute_output_shape([2, 3, 8, 8]) == [2, 32, 4, 4]
    m2 = Sequential.load_from_config(json.loads(json.dumps(m.get_config())))
    assert [x.type() for x in m2.layers] == ["conv2d", "grouped_conv2d"]
    assert m2.layers[1].get_config().parameters == m.layers[1].get_config().parameters


def test_constructor_rejections():
    from dcnn_amd.nn import GroupedConv2D
    with pytest.raises(ValueError, match="use Conv2D"):
        GroupedConv2D(16, 32, 3, 3, 1)
    with pytest.raises(ValueError, match="use DepthwiseConv2D"):
        GroupedConv2D(16, 16, 3, 3, 16)
    with pytest.raises(ValueError, match="groups 3 must divide"):
        GroupedConv2D(16, 32, 3, 3, 3)
    GroupedConv2D(16, 32, 3, 3, 16)  # channel multiplier 2: grouped, not depthwise


def test_init_rule_and_generator_order():
    """uniform +-1/sqrt(Cig*KH*KW), weights drawn before the bias from the layer's generator (Conv2D's order)."""
    from dcnn_amd.nn import GroupedConv2D
    l = GroupedConv2D(64, 128, 3, 3, 16, use_bias=True)
    l.set_seed(5)
    l.initialize()
    w, b = l.parameters()
    assert tuple(w.shape) == (128, 4, 3, 3) and tuple(b.shape) == (128, 1, 1, 1)
    bound = 1 / 6
    assert w.abs().max() <= bound and w.abs().max() > 0.9 * bound and b.abs().max() <= bound
    g = torch.Generator().manual_seed(5)
    assert torch.equal(w, torch.empty(128, 4, 3, 3).uniform_(-bound, bound, generator=g))
    assert torch.equal(b, torch.empty(128, 1, 1, 1).uniform_(-bound, bound, generator=g))


def test_layer_matches_autograd_and_honours_input_grad_flag():
    from dcnn_amd.nn import GroupedConv2D
    torch.manual_seed(3)
    l = GroupedConv2D(8, 16, 3, 3, 2, 2, 2, 1, 1, True, "g")
    l.set_seed(2)
    l.initialize()
    x = torch.randn(3, 8, 7, 6, requires_grad=True)
    w, b = [p.detach().clone().requires_grad_() for p in l.parameters()]
    ref = F.conv2d(x, w, b.view(-1), 2, 1, groups=2)
    dy = torch.randn_like(ref)
    ref.backward(dy)
    y = l.forward(x.detach(), 1)  # micro-batch 1 keeps its own cached input
    assert torch.allclose(y, ref.detach(), rtol=1e-5, atol=1e-6)
    add = torch.randn(3, 8, 7, 6)
    dx = l.backward(dy, 1, add_to=add)
    assert torch.allclose(dx, x.grad + add, rtol=1e-5, atol=1e-5)
    gw, gb = l.gradients()
    assert torch.allclose(gw, w.grad, rtol=1e-5, atol=1e-5) and torch.allclose(gb, b.grad, rtol=1e-5, atol=1e-5)
    with pytest.raises(RuntimeError, match="^GroupedConv2D 'g': no cached input for micro-batch 1$"):
        l.backward(dy, 1)
    l.needs_input_grad = False
    l.forward(x.detach())
    assert l.backward(dy) is None
    # the shared base's messages carry the concrete class name
    with pytest.raises(ValueError, match="^GroupedConv2D 'g': input has 4 channels, expected 8$"):
        l.forward(torch.randn(1, 4, 7, 6))
    with pytest.raises(RuntimeError, match="^GroupedConv2D 'cold' must be initialized before forward$"):
        GroupedConv2D(8, 16, 3, 3, 2, name="cold").forward(torch.randn(1, 8, 7, 6))


def _small_net():
    from dcnn_amd.nn import SequentialBuilder
    b = SequentialBuilder("gc_small").input([3, 16, 16])
    b.conv2d(32, 3, 3, 1, 1, 1, 1, False, "conv1").batchnorm(1e-5, 0.1, True, "bn1").activation("relu", "relu1")
    b.resnext_bottleneck_block(32, 32, 64, 8, 1, "block1").resnext_bottleneck_block(64, 64, 128, 8, 2, "block2")
    b.grouped_conv2d(64, 1, 1, 4, 1, 1, 0, 0, True, "gpw")
    return b.avgpool2d(8, 8, 1, 1, 0, 0, "avgpool").flatten("flatten").dense(10, True, "fc").build()


def test_resnext_block_structure():
    from dcnn_amd.nn import GroupedConv2D
    from dcnn_amd.nn.layers import Conv2D
    m = _small_net()
    blk = m.layers[3]
    assert blk.type() == "residual_block" and blk.name == "block1"
    assert [l.type() for l in blk.main_path] == ["conv2d", "batchnorm", "activation", "grouped_conv2d", "batchnorm",
                                                 "activation", "conv2d", "batchnorm"]
    g = blk.main_path[3]
    assert isinstance(g, GroupedConv2D) and not isinstance(g, Conv2D)
    assert (g.in_channels, g.out_channels, g.groups, g.kernel_h, g.stride_h, g.pad_h, g.use_bias) == \
        (32, 32, 8, 3, 1, 1, False)
    assert [l.type() for l in blk.shortcut_path] == ["conv2d", "batchnorm"]
    g2 = m.layers[4].main_path[3]
    assert (g2.in_channels, g2.groups, g2.stride_h, g2.stride_w) == (64, 8, 2, 2)
    assert m.compute_output_shape([2, 3, 16, 16]) == [2, 10, 1, 1]


def test_checkpoint_roundtrip_bit_exact(tmp_path):
    from dcnn_amd.nn import Adam, Sequential, load_checkpoint, save_checkpoint
    m = _small_net()
    m.set_seed(8)
    m.initialize()
    path = str(tmp_path / "gc_model")
    m.save_to_file(path)
    cfg = json.load(open(path + ".json"))
    gl = [l for l in cfg["layers"] if l["type"] == "grouped_conv2d"]
    assert [l["name"] for l in gl] == ["gpw"] and gl[0]["parameters"]["groups"] == 4
    # .bin: {u64 shape[4]; f32 data} per parameter in parameter order — no format change
    n = sum(32 + 4 * p.numel() for p in m.parameters())
    assert len(open(path + ".bin", "rb").read()) == n
    m2 = Sequential.from_file(path)
    assert [l.type() for l in m2.layers] == [l.type() for l in m.layers]
    assert m2.layers[3].main_path[3].get_config().parameters == m.layers[3].main_path[3].get_config().parameters
    for a, b in zip(m.parameters(), m2.parameters()):
        assert a.shape == b.shape and torch.equal(a, b)
    x = torch.randn(2, 3, 16, 16)
    m.set_training(False)
    m2.set_training(False)
    assert torch.equal(m.forward(x), m2.forward(x))
    # .state sidecar through save_checkpoint / load_checkpoint
    opt = Adam(1e-3)
    opt.attach(m)
    ck = str(tmp_path / "gc_ckpt")
    save_checkpoint(m, opt, ck, epoch=3)
    m3 = _small_net()
    m3.set_seed(99)
    m3.initialize()
    assert load_checkpoint(m3, None, ck) == 3
    m3.set_training(False)
    assert torch.equal(m.forward(x), m3.forward(x))


@pytest.mark.parametrize("name,blocks", [("resnext26_32x4d_cifar10", (2, 2, 2, 2)),
                                         ("resnext50_32x4d_tiny_imagenet", (3, 4, 6, 3))])
def test_resnext_zoo_models(name, blocks):
    from dcnn_amd.models import INPUT_SHAPES, MODELS, NUM_CLASSES, create_model
    from dcnn_amd.nn import GroupedConv2D
    assert name in MODELS
    m = create_model(name)
    C, H, W = INPUT_SHAPES[name]
    assert (C, H, W) == ((3, 32, 32) if "cifar" in name else (3, 64, 64))
    assert NUM_CLASSES[name] == (10 if "cifar" in name else 200)
    assert m.compute_output_shape([2, C, H, W]) == [2, NUM_CLASSES[name], 1, 1]
    gs = [l.main_path[3] for l in m.layers if l.type() == "residual_block"]
    assert len(gs) == sum(blocks) and all(isinstance(l, GroupedConv2D) for l in gs)
    want = []
    for s, (n, mid) in enumerate(zip(blocks, (128, 256, 512, 1024))):
        want += [(mid, mid, 32, 2 if (i == 0 and s > 0) else 1) for i in range(n)]
    assert [(l.in_channels, l.out_channels, l.groups, l.stride_h) for l in gs] == want
    assert all((l.kernel_h, l.kernel_w, l.pad_h, l.pad_w, l.use_bias) == (3, 3, 1, 1, False) for l in gs)
    names = [l.name for l in m.layers if l.type() == "residual_block"]
    assert names[0] == "layer1_block1" and names[-1] == f"layer4_block{blocks[3]}"


def test_resnext26_trains_on_cpu():
    """One training step at batch 2 has a finite loss, and the loss drops over 3 steps on a fixed batch."""
    from dcnn_amd.models import create_model
    from dcnn_amd.nn import Adam, GroupedConv2D, LossFactory
    torch.manual_seed(0)
    m = create_model("resnext26_32x4d_cifar10")
    assert sum(isinstance(l.main_path[3], GroupedConv2D) for l in m.layers if l.type() == "residual_block") == 8
    m.set_seed(4)
    m.initialize()
    opt = Adam(1e-3)
    opt.attach(m)
    lf = LossFactory.create("softmax_crossentropy")
    x = torch.randn(2, 3, 32, 32)
    y = torch.tensor([3, 7])
    losses = []
    for _ in range(3):
        m.clear_gradients()
        out = m.forward(x)
        loss, grad, _ = lf.loss_and_grad(out, y)
        m.backward(grad)
        opt.update()
        losses.append(float(loss))
    assert all(v == v and abs(v) < float("inf") for v in losses), losses
    assert losses[-1] < losses[0], losses
