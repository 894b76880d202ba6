"""Channel LayerNorm, LayerScale and GELU on the native CPU backend and the layer plumbing (factory,
builders, checkpoints, the ConvNeXt block, the scale-tail planner rule and the zoo models). Oracle:
F.layer_norm over the channel dimension, F.gelu and autograd."""
import json

import pytest
import torch
import torch.nn.functional as F

# (N, C, H, W) or (N, F)
SHAPES = [(1, 8, 1, 1), (2, 5, 3, 1), (3, 40, 2, 3), (2, 96, 4, 4), (4, 16), (2, 24, 3, 5)]
_ids = ["x".join(map(str, s)) for s in SHAPES]
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])


def rel(a, r):
    return ((a - r).norm() / (r.norm() + 1e-300)).item()


def chan_last(t):
    return t.permute(0, 2, 3, 1) if t.dim() == 4 else t


def chan_first(t):
    return t.permute(0, 3, 1, 2) if t.dim() == 4 else t


@DTYPES
@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_native_layernorm_matches_torch(shape, affine, dtype):
    from dcnn_amd.ops import cpu
    C = shape[1]
    tol = 1e-5 if dtype == torch.float32 else 1e-12
    g = torch.Generator().manual_seed(99)
    x = torch.randn(shape, dtype=dtype, generator=g, requires_grad=True)
    gamma = (1 + 0.5 * torch.randn(C, dtype=dtype, generator=g)).requires_grad_()
    beta = torch.randn(C, dtype=dtype, generator=g, requires_grad=True)
    ref = chan_first(F.layer_norm(chan_last(x), (C,), gamma if affine else None, beta if affine else None, 1e-6))
    dy = torch.randn(shape, dtype=dtype, generator=g)
    ref.backward(dy)
    y, mean, rstd = cpu.layernorm_fwd(x.detach(), gamma.detach() if affine else None,
                                      beta.detach() if affine else None, 1e-6)
    assert y.dtype == dtype and y.shape == x.shape and rel(y, ref.detach()) < tol
    xl = chan_last(x.detach()).reshape(-1, C)
    assert mean.shape == (xl.shape[0],) and rel(mean, xl.mean(1)) < tol
    assert rel(rstd, 1 / torch.sqrt(xl.var(1, unbiased=False) + 1e-6)) < tol
    dg = torch.full((C,), 0.5, dtype=dtype) if affine else None  # the gradients accumulate
    db = torch.full((C,), -2.0, dtype=dtype) if affine else None
    dx = cpu.layernorm_bwd(x.detach(), dy, gamma.detach() if affine else None, mean, rstd, dg, db)
    assert rel(dx, x.grad) < 10 * tol
    if affine:
        assert rel(dg, gamma.grad + 0.5) < 10 * tol and rel(db, beta.grad - 2.0) < 10 * tol


@DTYPES
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_native_layer_scale_and_gelu_match_torch(shape, dtype):
    from dcnn_amd.ops import cpu
    C = shape[1]
    tol = 1e-6 if dtype == torch.float32 else 1e-14
    g = torch.Generator().manual_seed(5)
    x = torch.randn(shape, dtype=dtype, generator=g, requires_grad=True)
    res = torch.randn(shape, dtype=dtype, generator=g)
    gamma = torch.randn(C, dtype=dtype, generator=g, requires_grad=True)
    bshape = (1, C) + (1,) * (len(shape) - 2)
    ref = x * gamma.view(bshape)
    dy = torch.randn(shape, dtype=dtype, generator=g)
    ref.backward(dy)
    assert rel(cpu.layer_scale_fwd(x.detach(), gamma.detach()), ref.detach()) < tol
    assert rel(cpu.layer_scale_fwd(x.detach(), gamma.detach(), res), ref.detach() + res) < tol
    dg = torch.full((C,), 0.5, dtype=dtype)
    dx = cpu.layer_scale_bwd(x.detach(), dy, gamma.detach(), dg)
    assert rel(dx, x.grad) < tol and rel(dg, gamma.grad + 0.5) < tol
    dg2 = torch.zeros(C, dtype=dtype)
    assert cpu.layer_scale_bwd(x.detach(), dy, gamma.detach(), dg2, need_dx=False) is None
    assert rel(dg2, gamma.grad) < tol
    # GELU (exact form): code 6 of the native act kernels, against F.gelu and autograd
    x2 = (3 * x.detach()).requires_grad_()
    yr = F.gelu(x2)
    yr.backward(dy)
    assert rel(cpu.act_fwd(x2.detach(), "gelu"), yr.detach()) < tol
    assert rel(cpu.act_bwd(x2.detach(), dy, "gelu"), x2.grad) < tol


def test_gelu_activation_registered():
    from dcnn_amd.nn import ActivationFactory
    from dcnn_amd.ops import cpu
    from dcnn_amd.ops.hip_layers import ACT_CODES
    assert "gelu" in ActivationFactory.get_available_activations()
    assert ACT_CODES == {"relu": 0, "leaky_relu": 1, "elu": 2, "sigmoid": 3, "tanh": 4, "linear": 5, "gelu": 6}
    assert cpu.ACT_CODES == {"linear": 0, "relu": 1, "leaky_relu": 2, "elu": 3, "sigmoid": 4, "tanh": 5, "gelu": 6}
    act = ActivationFactory.create("gelu")
    x = torch.linspace(-8, 8, 4099, dtype=torch.float64)
    g = torch.randn(4099, dtype=torch.float64)
    y = act.apply(x)
    assert rel(y, act._cpu(x)) < 1e-14 and rel(act.gradient(x, y, g), act._cpu_grad(x, y, g)) < 1e-14
    xr = x.clone().requires_grad_()
    F.gelu(xr).backward(g)
    assert rel(act._cpu_grad(x, y, g), xr.grad) < 1e-14


def _small_net():
    """input 3x16x16, stem 2x2 s2 -> 16 channels, one block, downsample -> 32, one block, head"""
    from dcnn_amd.nn import SequentialBuilder
    return (SequentialBuilder("convnext_small").input([3, 16, 16])
            .conv2d(16, 2, 2, 2, 2, 0, 0, True, "stem_conv").layernorm(1e-6, True, "stem_ln")
            .convnext_block(16, 0.5, "block1")
            .convnext_downsample(32, "down2")
            .convnext_block(32, 0.5, "block2")
            .avgpool2d(4, 4, 1, 1, 0, 0, "avgpool").layernorm(1e-6, True, "head_ln").flatten("flatten")
            .dense(10, True, "fc").build())


def test_config_roundtrip_factory_and_builders():
    from dcnn_amd.nn import LayerBuilder, LayerFactory, LayerNorm, LayerScale, create_layer
    assert {"layernorm", "layer_scale"} <= set(LayerFactory.available_types())
    ln = LayerNorm(24, 1e-5, False, "ln")
    c = ln.get_config()
    assert c.parameters == dict(num_channels=24, epsilon=1e-5, affine=False)
    ln2 = create_layer("layernorm", c)
    assert isinstance(ln2, LayerNorm) and ln2.get_config() == c and not ln2.has_parameters()
    assert LayerNorm(8).epsilon == 1e-6 and LayerNorm(8).affine and LayerNorm(8).name == "layernorm"
    ls = LayerScale(24, 0.25, "ls")
    c = ls.get_config()
    assert c.parameters == dict(num_channels=24, init_value=0.25)
    ls2 = create_layer("layer_scale", c)
    assert isinstance(ls2, LayerScale) and ls2.get_config() == c
    assert LayerScale(8).init_value == 1e-6 and LayerScale(8).name == "layer_scale"
    ls.initialize()
    ln3 = LayerNorm(24)
    ln3.initialize()
    assert [tuple(p.shape) for p in ls.parameters()] == [(24, 1, 1, 1)] and torch.all(ls.parameters()[0] == 0.25)
    assert [tuple(p.shape) for p in ln3.parameters()] == [(24, 1, 1, 1)] * 2
    assert torch.all(ln3.parameters()[0] == 1) and torch.all(ln3.parameters()[1] == 0)
    layers = LayerBuilder().input([24, 4, 4]).layernorm().layer_scale(0.1).build()
    assert [l.type() for l in layers] == ["layernorm", "layer_scale"]
    assert [l.name for l in layers] == ["layernorm_0", "layer_scale_1"]
    assert layers[0].num_channels == 24 and layers[1].num_channels == 24 and layers[1].init_value == 0.1
    with pytest.raises(ValueError, match="LayerNorm"):
        ln3.forward(torch.zeros(2, 8, 4, 4))


def test_layers_match_autograd():
    """LayerNorm and LayerScale layers (4-D and 2-D inputs) against autograd; gradients accumulate."""
    from dcnn_amd.nn import LayerNorm, LayerScale
    torch.manual_seed(3)
    for shape in [(2, 24, 3, 5), (4, 24)]:
        ln, ls = LayerNorm(24), LayerScale(24, 0.5)
        for l in (ln, ls):
            l.set_seed(1)
            l.initialize()
        ln.parameters()[0].copy_(1 + 0.3 * torch.randn(24, 1, 1, 1))
        ln.parameters()[1].copy_(torch.randn(24, 1, 1, 1))
        x = torch.randn(shape, requires_grad=True)
        res = torch.randn(shape)
        gm, bt = (p.detach().view(-1).clone().requires_grad_() for p in ln.parameters())
        sc = ls.parameters()[0].detach().view(-1).clone().requires_grad_()
        bshape = (1, 24) + (1,) * (len(shape) - 2)
        ref = chan_first(F.layer_norm(chan_last(x), (24,), gm, bt, 1e-6)) * sc.view(bshape) + res
        dy = torch.randn(shape)
        ref.backward(dy)
        y = ls.forward(ln.forward(x.detach()), 0, residual=res)
        assert rel(y, ref.detach()) < 1e-5
        dx = ln.backward(ls.backward(dy))
        assert rel(dx, x.grad) < 1e-5
        assert rel(ln.gradients()[0].view(-1), gm.grad) < 1e-5 and rel(ln.gradients()[1].view(-1), bt.grad) < 1e-5
        assert rel(ls.gradients()[0].view(-1), sc.grad) < 1e-5
        with pytest.raises(RuntimeError, match="no cached data"):
            ln.backward(dy)


def test_convnext_block_structure():
    m = _small_net()
    assert [l.type() for l in m.layers] == ["conv2d", "layernorm", "residual_block", "layernorm", "conv2d",
                                            "residual_block", "avgpool2d", "layernorm", "flatten", "dense"]
    assert [l.name for l in m.layers[3:5]] == ["down2_ln", "down2_conv"]
    d = m.layers[4]
    assert (d.in_channels, d.out_channels, d.kernel_h, d.stride_h, d.pad_h, d.use_bias) == (16, 32, 2, 2, 0, True)
    blk = m.layers[2]
    assert blk.name == "block1" and blk.activation_type == "none" and blk.shortcut_path == []
    assert [l.type() for l in blk.main_path] == ["depthwise_conv2d", "layernorm", "conv2d", "activation", "conv2d",
                                                 "layer_scale"]
    assert [l.name for l in blk.main_path] == ["depthwise_conv2d_0", "layernorm_1", "conv2d_2", "activation_3",
                                               "conv2d_4", "layer_scale_5"]
    dw, ln, pw1, act, pw2, ls = blk.main_path
    assert (dw.in_channels, dw.kernel_h, dw.kernel_w, dw.stride_h, dw.pad_h, dw.pad_w, dw.use_bias) == \
        (16, 7, 7, 1, 3, 3, True)
    assert (ln.num_channels, ln.epsilon, ln.affine) == (16, 1e-6, True)
    assert (pw1.in_channels, pw1.out_channels, pw1.kernel_h, pw1.use_bias) == (16, 64, 1, True)
    assert act.activation_name == "gelu"
    assert (pw2.in_channels, pw2.out_channels, pw2.kernel_h, pw2.use_bias) == (64, 16, 1, True)
    assert (ls.num_channels, ls.init_value) == (16, 0.5)
    assert m.compute_output_shape([2, 3, 16, 16]) == [2, 10, 1, 1]


def test_checkpoint_roundtrip_bit_exact(tmp_path):
    from dcnn_amd.nn import Sequential
    m = _small_net()
    m.set_seed(8)
    m.initialize()
    path = str(tmp_path / "cnx_model")
    m.save_to_file(path)
    cfg = json.load(open(path + ".json"))
    assert [l["name"] for l in cfg["layers"] if l["type"] == "layernorm"] == ["stem_ln", "down2_ln", "head_ln"]
    # .bin: {u64 shape[4]; f32 data} per parameter in parameter order — no format change
    n = sum(32 + 4 * p.numel() for p in m.parameters())
    assert len(open(path + ".bin", "rb").read()) == n
    m2 = Sequential.from_file(path)
    assert [l.type() for l in m2.layers] == [l.type() for l in m.layers]
    for a, b in zip(m.layers[2].main_path, m2.layers[2].main_path):
        assert a.type() == b.type() and a.get_config().parameters == b.get_config().parameters
    for a, b in zip(m.parameters(), m2.parameters()):
        assert a.shape == b.shape and torch.equal(a, b)
    x = torch.randn(2, 3, 16, 16)
    m.set_training(False)
    m2.set_training(False)
    assert torch.equal(m.forward(x), m2.forward(x))


def test_small_net_matches_autograd():
    """The whole small ConvNeXt on the CPU (float64) against the same network written in PyTorch."""
    m = _small_net()
    m.set_seed(2)
    m.set_compute_dtype(torch.float64)
    m.initialize()
    ps = [p.detach().clone().requires_grad_() for p in m.parameters()]
    it = iter(ps)

    def ln(t):
        g, b = next(it), next(it)
        return chan_first(F.layer_norm(chan_last(t), (t.shape[1],), g.view(-1), b.view(-1), 1e-6))

    def block(t):
        w, b = next(it), next(it)
        h = F.conv2d(t, w, b.view(-1), padding=3, groups=t.shape[1])
        h = ln(h)
        w, b = next(it), next(it)
        h = F.gelu(F.conv2d(h, w, b.view(-1)))
        w, b = next(it), next(it)
        h = F.conv2d(h, w, b.view(-1))
        return t + h * next(it).view(1, -1, 1, 1)

    x = torch.randn(2, 3, 16, 16, dtype=torch.float64, requires_grad=True)
    w, b = next(it), next(it)
    h = block(ln(F.conv2d(x, w, b.view(-1), stride=2)))
    h = ln(h)
    w, b = next(it), next(it)
    h = block(F.conv2d(h, w, b.view(-1), stride=2))
    h = ln(F.avg_pool2d(h, 4)).flatten(1)
    w, b = next(it), next(it)
    ref = F.linear(h, w.view(w.shape[0], -1), b.view(-1))
    dy = torch.randn(2, 10, dtype=torch.float64)
    ref.backward(dy)
    y = m.forward(x.detach())
    assert rel(y.reshape(2, 10), ref.detach()) < 1e-12
    m.clear_gradients()
    dx = m.backward(dy.view(y.shape))
    assert rel(dx, x.grad) < 1e-11
    for g, p in zip(m.gradients(), ps):
        assert rel(g.reshape(-1), p.grad.reshape(-1)) < 1e-11


def test_scale_tail_planner_rule():
    """RF_SCALE_TAIL: main path closing in a LayerScale, identity shortcut, no activation — only."""
    from dcnn_amd.nn.layers.residual import fuse_kinds
    from dcnn_amd.ops._ext import kernels
    K = kernels()
    assert (K.FK_LSCALE, K.RF_SCALE_TAIL) == (9, 4)
    C, B, A, O, L = K.FK_CONV, K.FK_BN, K.FK_ACT, K.FK_OTHER, K.FK_LSCALE
    blk = _small_net().layers[2]
    kinds = fuse_kinds(blk.main_path)
    assert kinds == [O, O, C, A, C, L]
    assert K.plan_residual_fusions(kinds, [], True, True) == K.RF_SCALE_TAIL       # none / linear
    assert K.plan_residual_fusions(kinds, [], True, False) == 0                   # relu
    assert K.plan_residual_fusions(kinds, [], True) == 0                          # (the default)
    assert K.plan_residual_fusions(kinds, [C, B], True, True) == 0                # projection shortcut
    assert K.plan_residual_fusions(kinds[:-1], [], True, True) == 0               # no LayerScale at the end
    assert K.plan_residual_fusions([L], [], True, True) == 0                      # one-layer main path
    assert K.plan_residual_fusions([C, B], [], True, True) == K.RF_FUSED_TAIL     # the BatchNorm tail as before
    assert K.plan_residual_fusions([C, B], [C, B], True, True) == K.RF_FUSED_TAIL | K.RF_DUAL_SHORTCUT
    assert K.plan_sequence_fusions(kinds) == [0] * 6
    assert not blk._scale_tail  # the CPU keeps the plain path


@pytest.mark.parametrize("name,patch,depths,widths,params", [
    ("convnext_pico_cifar10", 2, (2, 2, 6, 2), (64, 128, 256, 512), 8535498),
    ("convnext_tiny_tiny_imagenet", 4, (3, 3, 9, 3), (96, 192, 384, 768), 27973928)])
def test_convnext_zoo_models(name, patch, depths, widths, params):
    """Structure, parameter count (that of a plain PyTorch ConvNeXt of the same widths: Conv2d / LayerNorm /
    Linear modules plus one layer-scale vector per block) and one CPU forward/backward at batch 2."""
    from dcnn_amd.models import INPUT_SHAPES, MODELS, NUM_CLASSES, create_model
    assert name in MODELS
    m = create_model(name)
    C, H, W = INPUT_SHAPES[name]
    assert (C, H, W) == ((3, 32, 32) if "cifar" in name else (3, 64, 64))
    assert NUM_CLASSES[name] == (10 if "cifar" in name else 200)
    assert m.compute_output_shape([2, C, H, W]) == [2, NUM_CLASSES[name], 1, 1]
    stem = m.layers[0]
    assert (stem.name, stem.in_channels, stem.out_channels, stem.kernel_h, stem.stride_h, stem.pad_h) == \
        ("stem_conv", 3, widths[0], patch, patch, 0)
    assert m.layers[1].type() == "layernorm" and m.layers[1].name == "stem_ln"
    blocks = [l for l in m.layers if l.type() == "residual_block"]
    want = [(f"stage{s}_block{i}", w) for s, (n, w) in enumerate(zip(depths, widths), 1) for i in range(1, n + 1)]
    assert [(b.name, b.main_path[0].in_channels) for b in blocks] == want
    assert all(b.activation_type == "none" and not b.shortcut_path and b.main_path[-1].init_value == 1e-6
               for b in blocks)
    downs = [l for l in m.layers if l.type() == "conv2d" and l.name.startswith("down")]
    assert [(d.name, d.out_channels, d.kernel_h, d.stride_h) for d in downs] == \
        [(f"down{s}_conv", widths[s - 1], 2, 2) for s in (2, 3, 4)]
    assert [l.name for l in m.layers[-4:]] == ["avgpool", "head_ln", "flatten", "fc"]
    assert (m.layers[-4].pool_h, m.layers[-4].pool_w) == (2, 2)
    m.set_seed(1)
    m.initialize()
    assert m.num_parameters() == params
    torch.manual_seed(0)
    x = torch.randn(2, C, H, W)
    y = m.forward(x)
    assert tuple(y.shape) == (2, NUM_CLASSES[name], 1, 1) and torch.isfinite(y).all()
    dx = m.backward(torch.randn_like(y))
    assert tuple(dx.shape) == (2, C, H, W) and torch.isfinite(dx).all()
    assert all(torch.isfinite(g).all() for g in m.gradients())
    assert any(g.abs().sum() > 0 for g in blocks[0].main_path[-1].gradients())
