"""Depthwise convolution on the native CPU backend and the DepthwiseConv2D layer plumbing (factory,
builders, checkpoints, MobileNetV1 zoo models). Oracle: F.conv2d(groups=C) and autograd."""
import json

import pytest
import torch
import torch.nn.functional as F

# the kernel cases of tests/test_gpu_dwconv.py minus the multi-split one:
# (N, C, H, W, (KH, KW), (SH, SW), (PH, PW))
CASES = [
    (1, 8, 1, 1, (3, 3), (1, 1), (1, 1)),
    (2, 32, 2, 2, (3, 3), (2, 2), (1, 1)),
    (2, 64, 16, 16, (3, 3), (1, 1), (1, 1)),
    (2, 64, 16, 16, (3, 3), (2, 2), (1, 1)),
    (3, 40, 7, 5, (3, 3), (1, 1), (1, 1)),
    (3, 40, 7, 5, (3, 3), (2, 2), (1, 1)),
    (2, 16, 8, 8, (3, 3), (2, 2), (0, 0)),
    (4, 512, 4, 4, (3, 3), (1, 1), (1, 1)),
    (2, 128, 9, 9, (3, 3), (2, 2), (1, 1)),
    (2, 32, 8, 8, (3, 3), (1, 1), (0, 0)),
    (2, 24, 12, 10, (5, 5), (1, 1), (2, 2)),
    (2, 16, 9, 9, (7, 7), (2, 2), (3, 3)),
    (2, 16, 10, 6, (1, 3), (1, 2), (0, 1)),
]
_ids = [f"n{c[0]}c{c[1]}_{c[2]}x{c[3]}_k{c[4][0]}x{c[4][1]}_s{c[5][0]}{c[5][1]}_p{c[6][0]}{c[6][1]}" for c in CASES]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_native_depthwise_matches_torch(case, dtype):
    from dcnn_amd.ops import cpu
    N, C, H, W, (KH, KW), st, pd = case
    rtol = 1e-5 if dtype == torch.float32 else 1e-12
    g = torch.Generator().manual_seed(7)
    x = torch.randn(N, C, H, W, dtype=dtype, generator=g, requires_grad=True)
    w = (torch.randn(C, 1, KH, KW, dtype=dtype, generator=g) / (KH * KW) ** 0.5).requires_grad_()
    b = torch.randn(C, dtype=dtype, generator=g, requires_grad=True)
    ref = F.conv2d(x, w, b, st, pd, groups=C)
    dy = torch.randn(ref.shape, dtype=dtype, generator=g)
    ref.backward(dy)

    def close(a, r):
        # rtol of the largest reference magnitude: cancelling sums carry the rounding of their terms
        return (a - r).abs().max().item() <= rtol * r.abs().max().item()

    y = cpu.depthwise_conv2d_fwd(x.detach(), w.detach(), b.detach(), st, pd)
    assert y.dtype == dtype and close(y, ref.detach())
    y0 = cpu.depthwise_conv2d_fwd(x.detach(), w.detach(), None, st, pd)
    assert close(y0, F.conv2d(x, w, None, st, pd, groups=C).detach())
    # accumulation into non-zero gradients
    gw = torch.full((C, 1, KH, KW), 0.5, dtype=dtype)
    gb = torch.full((C,), -2.0, dtype=dtype)
    dx = cpu.depthwise_conv2d_bwd(x.detach(), w.detach(), dy, st, pd, gw, gb)
    assert close(dx, x.grad) and close(gw, w.grad + 0.5) and close(gb, b.grad - 2.0)
    # need_dx=False: parameter gradients only
    gw2 = torch.zeros(C, 1, KH, KW, dtype=dtype)
    assert cpu.depthwise_conv2d_bwd(x.detach(), w.detach(), dy, st, pd, gw2, None, need_dx=False) is None
    assert close(gw2, w.grad)


def test_layer_config_roundtrip_factory_and_builders():
    from dcnn_amd.nn import DepthwiseConv2D, LayerFactory, Sequential, SequentialBuilder
    from dcnn_amd.nn.layers import Conv2D, LayerBuilder, create_layer
    assert "depthwise_conv2d" in LayerFactory.available_types()
    l = DepthwiseConv2D(24, 5, 3, 2, 1, 2, 1, False, "dwx")
    assert not isinstance(l, Conv2D) and l.type() == "depthwise_conv2d"
    cfg = l.get_config()
    assert cfg.parameters == dict(channels=24, kernel_h=5, kernel_w=3, stride_h=2, stride_w=1, pad_h=2, pad_w=1,
                                  use_bias=False)
    again = create_layer("depthwise_conv2d", cfg)
    assert isinstance(again, DepthwiseConv2D) and again.get_config().parameters == cfg.parameters
    assert again.name == "dwx"
    assert l.compute_output_shape([4, 24, 11, 9]) == [4, 24, 6, 9]
    assert l.forward_flops([4, 24, 11, 9]) == 2 * 24 * 15 * 4 * 6 * 9
    assert l.backward_flops([4, 24, 11, 9]) == 2 * l.forward_flops([4, 24, 11, 9])
    assert DepthwiseConv2D(8, 3, 3).forward_flops([1, 8, 4, 4]) == 2 * 8 * 9 * 4 + 8 * 4
    assert [tuple(s.shape) for s in DepthwiseConv2D(8, 3, 3).param_specs()] == [(8, 1, 3, 3), (8, 1, 1, 1)]
    # builders infer the channel count from the running shape
    lb = LayerBuilder().input([12, 8, 8]).depthwise_conv2d(3, 3, 2, 2, 1, 1, True, "a").build()
    assert lb[0].channels == 12 and lb[0].use_bias
    m = SequentialBuilder("s").input([3, 8, 8]).conv2d(16, 3, 3, 1, 1, 1, 1).depthwise_conv2d(3, 3, 2, 2, 1, 1).build()
    assert m.layers[1].channels == 16 and m.compute_output_shape([2, 3, 8, 8]) == [2, 16, 4, 4]
    m2 = Sequential.load_from_config(json.loads(json.dumps(m.get_config())))
    assert [x.type() for x in m2.layers] == ["conv2d", "depthwise_conv2d"]
    assert m2.layers[1].get_config().parameters == m.layers[1].get_config().parameters


def test_init_rule_and_generator_order():
    """uniform +-1/sqrt(KH*KW), weights drawn before the bias from the layer's generator (Conv2D's order)."""
    from dcnn_amd.nn import DepthwiseConv2D
    l = DepthwiseConv2D(64, 3, 3, use_bias=True)
    l.set_seed(5)
    l.initialize()
    w, b = l.parameters()
    assert tuple(w.shape) == (64, 1, 3, 3) and tuple(b.shape) == (64, 1, 1, 1)
    assert w.abs().max() <= 1 / 3 and w.abs().max() > 0.9 / 3 and b.abs().max() <= 1 / 3
    g = torch.Generator().manual_seed(5)
    assert torch.equal(w, torch.empty(64, 1, 3, 3).uniform_(-1 / 3, 1 / 3, generator=g))
    assert torch.equal(b, torch.empty(64, 1, 1, 1).uniform_(-1 / 3, 1 / 3, generator=g))


def _small_net():
    from dcnn_amd.nn import SequentialBuilder
    b = SequentialBuilder("dw_small").input([3, 16, 16])
    b.conv2d(16, 3, 3, 1, 1, 1, 1, False, "conv1").batchnorm(1e-5, 0.1, True, "bn1").activation("relu", "relu1")
    for i, (co, s) in enumerate(((32, 1), (64, 2)), 1):
        (b.depthwise_conv2d(3, 3, s, s, 1, 1, i == 2, f"dw{i}").batchnorm(1e-5, 0.1, True, f"dw{i}_bn")
         .activation("relu", f"dw{i}_relu")
         .conv2d(co, 1, 1, 1, 1, 0, 0, False, f"pw{i}").batchnorm(1e-5, 0.1, True, f"pw{i}_bn")
         .activation("relu", f"pw{i}_relu"))
    return b.avgpool2d(8, 8, 1, 1, 0, 0, "avgpool").flatten("flatten").dense(10, True, "fc").build()


def test_layer_matches_autograd_and_honours_input_grad_flag():
    from dcnn_amd.nn import DepthwiseConv2D
    torch.manual_seed(3)
    l = DepthwiseConv2D(8, 3, 3, 2, 2, 1, 1, True, "dw")
    l.set_seed(2)
    l.initialize()
    x = torch.randn(3, 8, 7, 6, requires_grad=True)
    w, b = [p.detach().clone().requires_grad_() for p in l.parameters()]
    ref = F.conv2d(x, w, b.view(-1), 2, 1, groups=8)
    dy = torch.randn_like(ref)
    ref.backward(dy)
    y = l.forward(x.detach(), 1)  # micro-batch 1 keeps its own cached input
    assert torch.allclose(y, ref.detach(), rtol=1e-5, atol=1e-6)
    add = torch.randn(3, 8, 7, 6)
    dx = l.backward(dy, 1, add_to=add)
    assert torch.allclose(dx, x.grad + add, rtol=1e-5, atol=1e-5)
    gw, gb = l.gradients()
    assert torch.allclose(gw, w.grad, rtol=1e-5, atol=1e-5) and torch.allclose(gb, b.grad, rtol=1e-5, atol=1e-5)
    with pytest.raises(RuntimeError, match="^DepthwiseConv2D 'dw': no cached input for micro-batch 1$"):
        l.backward(dy, 1)
    l.needs_input_grad = False
    l.forward(x.detach())
    assert l.backward(dy) is None
    # the shared base's messages carry the concrete class name
    with pytest.raises(ValueError, match="^DepthwiseConv2D 'dw': input has 4 channels, expected 8$"):
        l.forward(torch.randn(1, 4, 7, 6))
    with pytest.raises(RuntimeError, match="^DepthwiseConv2D 'cold' must be initialized before forward$"):
        DepthwiseConv2D(8, 3, 3, name="cold").forward(torch.randn(1, 8, 7, 6))


def test_checkpoint_roundtrip_bit_exact(tmp_path):
    from dcnn_amd.nn import Sequential
    m = _small_net()
    m.set_seed(8)
    m.initialize()
    path = str(tmp_path / "dw_model")
    m.save_to_file(path)
    cfg = json.load(open(path + ".json"))
    dw = [l for l in cfg["layers"] if l["type"] == "depthwise_conv2d"]
    assert [l["name"] for l in dw] == ["dw1", "dw2"] and dw[0]["parameters"]["channels"] == 16
    # .bin: {u64 shape[4]; f32 data} per parameter in parameter order — no format change
    n = sum(32 + 4 * p.numel() for p in m.parameters())
    assert len(open(path + ".bin", "rb").read()) == n
    m2 = Sequential.from_file(path)
    assert [l.type() for l in m2.layers] == [l.type() for l in m.layers]
    for a, b in zip(m.parameters(), m2.parameters()):
        assert a.shape == b.shape and torch.equal(a, b)
    x = torch.randn(2, 3, 16, 16)
    m.set_training(False)
    m2.set_training(False)
    assert torch.equal(m.forward(x), m2.forward(x))


@pytest.mark.parametrize("name", ["mobilenet_v1_cifar10", "mobilenet_v1_tiny_imagenet"])
def test_mobilenet_zoo_models(name):
    from dcnn_amd.models import INPUT_SHAPES, MODELS, NUM_CLASSES, create_model
    from dcnn_amd.nn import DepthwiseConv2D
    assert name in MODELS
    m = create_model(name)
    C, H, W = INPUT_SHAPES[name]
    assert (C, H, W) == ((3, 32, 32) if "cifar" in name else (3, 64, 64))
    assert NUM_CLASSES[name] == (10 if "cifar" in name else 200)
    assert m.compute_output_shape([2, C, H, W]) == [2, NUM_CLASSES[name], 1, 1]
    dws = [l for l in m.layers if isinstance(l, DepthwiseConv2D)]
    assert len(dws) == 13
    assert [(l.channels, l.stride_h) for l in dws] == [(32, 1), (64, 2), (128, 1), (128, 2), (256, 1), (256, 2)] + \
        [(512, 1)] * 5 + [(512, 2), (1024, 1)]
    assert all((l.kernel_h, l.kernel_w, l.pad_h, l.pad_w, l.use_bias) == (3, 3, 1, 1, False) for l in dws)
    m.set_seed(1)
    m.initialize()
    assert 3.1e6 <= m.num_parameters() <= 3.5e6, m.num_parameters()
    y = m.forward(torch.randn(2, C, H, W))
    assert y.shape == (2, NUM_CLASSES[name], 1, 1) and torch.isfinite(y).all()
    assert m.forward_flops([1, C, H, W]) > 0


def test_training_decreases_loss():
    from dcnn_amd.nn import Adam, LossFactory
    torch.manual_seed(0)
    m = _small_net()
    m.set_seed(4)
    m.initialize()
    opt = Adam(3e-3)
    opt.attach(m)
    lf = LossFactory.create("softmax_crossentropy")
    x = torch.randn(16, 3, 16, 16)
    y = torch.randint(0, 10, (16,))
    losses = []
    for _ in range(8):
        m.clear_gradients()
        out = m.forward(x)
        loss, grad, _ = lf.loss_and_grad(out, y)
        m.backward(grad)
        opt.update()
        losses.append(float(loss))
    assert losses[-1] < losses[0] and all(v == v for v in losses), losses
