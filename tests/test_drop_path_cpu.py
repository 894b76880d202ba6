"""DropPath (stochastic depth) on the CPU: the layer's semantics, the mask function, a float64 ConvNeXt
block with a DropPath against torch autograd given the layer's own mask, the JSON round trip and the
zoo's ``drop_path_rate``."""
import json

import pytest
import torch
import torch.nn.functional as F


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _layer(p, seed=None, set_seed=None, dtype=torch.float32):
    from dcnn_amd.nn.layers import DropPath
    l = DropPath(p, "dp", seed)
    if set_seed is not None:
        l.set_seed(set_seed)
    l.set_compute_dtype(dtype)
    return l


def test_identity_in_eval_and_at_rate_zero():
    x = torch.randn(5, 3, 2, 2)
    for l in (_layer(0.0), _layer(0.5)):
        if l.drop_rate > 0:
            l.set_training(False)
        y = l.forward(x)
        assert y is x and torch.equal(y, x)
        g = torch.randn_like(x)
        assert l.backward(g) is g


@pytest.mark.parametrize("p", [-0.1, 1.0, 1.5])
def test_rate_outside_range_raises(p):
    from dcnn_amd.nn.layers import DropPath
    with pytest.raises(ValueError):
        DropPath(p)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("shape", [(6, 3, 4, 5), (7, 9)])
def test_forward_backward_use_the_mask(shape, dtype):
    p = 0.5
    l = _layer(p, seed=11, dtype=dtype)
    x, dy = torch.randn(shape, dtype=dtype), torch.randn(shape, dtype=dtype)
    y = l.forward(x)
    m = l.last_mask()
    assert m.dtype == torch.float32 and tuple(m.shape) == (shape[0],)
    keep = torch.tensor(1.0 / (1.0 - p), dtype=torch.float32)
    assert all(v == 0.0 or v == keep for v in m)
    mv = m.to(dtype).view(-1, *([1] * (len(shape) - 1)))
    assert y.dtype == dtype and torch.equal(y, x * mv)
    dx = l.backward(dy)
    assert torch.equal(dx, dy * mv)


def test_mask_values_at_another_rate():
    m = _mask(5, 1, 64, 0.1)
    keep = torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - torch.tensor(0.1))
    assert set(m.tolist()) <= {0.0, keep.item()}


def _mask(seed, draw, n, p):
    from dcnn_amd.ops import cpu
    return cpu.drop_path_mask(seed, draw, n, p)


def test_same_seed_same_sequence_and_draws_differ():
    a, b = _layer(0.5, seed=77), _layer(0.5, set_seed=77)  # explicit and derived: the same function
    x = torch.randn(64, 2)
    seq = []
    for k in range(4):
        a.forward(x)
        b.forward(x)
        assert torch.equal(a.last_mask(), b.last_mask())
        assert torch.equal(a.last_mask(), _mask(77, k + 1, 64, 0.5))  # draw index = forwards so far, from 1
        seq.append(a.last_mask())
    for i in range(4):
        for j in range(i + 1, 4):
            assert not torch.equal(seq[i], seq[j])
    c = _layer(0.5, seed=78)
    c.forward(x)
    assert not torch.equal(c.last_mask(), seq[0])


def test_explicit_seed_overrides_the_derived_one():
    a = _layer(0.5, seed=5, set_seed=123)
    a.forward(torch.randn(32, 2))
    assert torch.equal(a.last_mask(), _mask(5, 1, 32, 0.5))


def test_mask_independent_of_shape_and_dtype():
    ms = []
    for shape, dtype in (((16, 3, 4, 4), torch.float32), ((16, 8), torch.float64), ((16, 1, 1, 1), torch.float32)):
        l = _layer(0.5, seed=9, dtype=dtype)
        l.forward(torch.randn(shape, dtype=dtype))
        ms.append(l.last_mask())
    assert torch.equal(ms[0], ms[1]) and torch.equal(ms[0], ms[2])
    assert torch.equal(_mask(9, 1, 16, 0.5)[:5], _mask(9, 1, 5, 0.5))  # m[n] does not depend on N


def test_two_microbatches_in_flight():
    l = _layer(0.5, seed=4)
    x0, x1 = torch.randn(64, 3), torch.randn(64, 3)
    l.forward(x0, 0)
    l.forward(x1, 1)
    m0, m1 = l.last_mask(0), l.last_mask(1)
    assert not torch.equal(m0, m1)
    dy = torch.ones(64, 3)
    assert torch.equal(l.backward(dy, 1), dy * m1.view(-1, 1))
    assert torch.equal(l.backward(dy, 0), dy * m0.view(-1, 1))


def test_keep_share():
    """N = 4096, p = 0.25: the kept share within 0.75 +- 0.04 (6 standard deviations of Binomial(4096, 0.75))."""
    m = _mask(20240607, 1, 4096, 0.25)
    share = (m != 0).float().mean().item()
    print(f"kept share {share:.4f}")
    assert abs(share - 0.75) <= 0.04


def _block_net(rate, seed, dtype=None):
    from dcnn_amd.nn import SequentialBuilder
    m = (SequentialBuilder("cnx_dp").input([8, 6, 6])
         .convnext_block(8, 0.5, "block1", drop_path=rate, drop_path_seed=seed).build())
    m.set_seed(3)
    if dtype is not None:
        m.set_compute_dtype(dtype)
    m.initialize()
    return m


def test_block_matches_autograd_float64():
    """x + m[n] gamma F(x) and every gradient against torch autograd given the layer's own mask
    (the bounds of tests/test_lnorm_cpu.py::test_small_net_matches_autograd)."""
    m = _block_net(0.5, 21, torch.float64)
    blk = m.layers[0]
    assert [l.type() for l in blk.main_path][-2:] == ["layer_scale", "drop_path"]
    N = 6
    x = torch.randn(N, 8, 6, 6, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(N, 8, 6, 6, dtype=torch.float64)
    y = m.forward(x.detach())
    mask = blk.main_path[-1].last_mask()
    assert 0 < int((mask != 0).sum()) < N, "seed 21 draws both kinds of sample"
    ps = [p.detach().clone().requires_grad_() for p in m.parameters()]
    it = iter(ps)
    w, b = next(it), next(it)
    h = F.conv2d(x, w, b.view(-1), padding=3, groups=8)
    g, b = next(it), next(it)
    h = F.layer_norm(h.permute(0, 2, 3, 1), (8,), g.view(-1), b.view(-1), 1e-6).permute(0, 3, 1, 2)
    w, b = next(it), next(it)
    h = F.gelu(F.conv2d(h, w, b.view(-1)))
    w, b = next(it), next(it)
    h = F.conv2d(h, w, b.view(-1))
    ref = x + h * next(it).view(1, -1, 1, 1) * mask.double().view(-1, 1, 1, 1)
    ref.backward(dy)
    assert rel(y, ref.detach()) < 1e-12
    m.clear_gradients()
    dx = m.backward(dy)
    assert rel(dx, x.grad) < 1e-11
    for gr, p in zip(m.gradients(), ps):
        assert rel(gr.reshape(-1), p.grad.reshape(-1)) < 1e-11


def test_json_round_trip(tmp_path):
    from dcnn_amd.nn import Sequential, SequentialBuilder
    from dcnn_amd.nn.layers import LayerBuilder
    m = (SequentialBuilder("dp_cfg").input([8, 6, 6])
         .convnext_block(8, 0.5, "block1", drop_path=0.25, drop_path_seed=(1 << 40) + 3)
         .drop_path(0.125, "dp_top")
         .flatten("flatten").dense(4, True, "fc").build())
    assert [l.type() for l in LayerBuilder().input([4, 2, 2]).drop_path(0.5).build()] == ["drop_path"]
    m.set_seed(5)
    m.initialize()
    path = str(tmp_path / "dp_model")
    m.save_to_file(path)
    cfg = json.load(open(path + ".json"))
    top = [l for l in cfg["layers"] if l["type"] == "drop_path"]
    assert len(top) == 1 and top[0]["parameters"] == {"drop_rate": 0.125}  # no explicit seed: none written
    inner = json.loads(cfg["layers"][0]["parameters"]["main_path"])[-1]
    assert inner["type"] == "drop_path" and inner["parameters"] == {"drop_rate": 0.25, "seed": (1 << 40) + 3}
    m2 = Sequential.from_file(path)
    d1, d2 = m.layers[0].main_path[-1], m2.layers[0].main_path[-1]
    assert (d2.drop_rate, d2.explicit_seed, d2.name) == (d1.drop_rate, d1.explicit_seed, d1.name)
    assert m2.layers[1].type() == "drop_path" and m2.layers[1].drop_rate == 0.125
    x = torch.randn(8, 8, 6, 6)
    m2.layers[0].forward(x)
    m.layers[0].forward(x)
    assert torch.equal(d1.last_mask(), d2.last_mask())
    c = m.clone()
    dc = c.layers[0].main_path[-1]
    assert dc.type() == "drop_path" and dc.explicit_seed == d1.explicit_seed and dc.drop_rate == 0.25
    assert m.forward_flops([2, 8, 6, 6]) > 0 and d1.forward_flops([2, 8, 6, 6]) == 2 * 8 * 6 * 6


def test_zoo_drop_path_rate():
    from dcnn_amd.models import create_model

    def names(m):
        out = []
        for l in m.layers:
            out.append(l.name)
            if l.type() == "residual_block":
                out += [s.name for s in l.main_path]
        return out

    def dps(m):
        return [s for l in m.layers if l.type() == "residual_block" for s in l.main_path if s.type() == "drop_path"]

    base = create_model("convnext_pico_cifar10")
    assert dps(base) == []
    blocks = [l for l in base.layers if l.type() == "residual_block"]
    assert len(blocks) == 12
    assert all([s.name for s in b.main_path] == ["depthwise_conv2d_0", "layernorm_1", "conv2d_2", "activation_3",
                                                   "conv2d_4", "layer_scale_5"] for b in blocks)
    assert names(create_model("convnext_pico_cifar10", drop_path_rate=0.0)) == names(base)
    m = create_model("convnext_pico_cifar10", drop_path_rate=0.1)
    d = dps(m)
    assert len(d) == 11
    assert [x.drop_rate for x in d] == pytest.approx([0.1 * i / 11 for i in range(1, 12)], rel=1e-12)
    mb = [l for l in m.layers if l.type() == "residual_block"]
    assert [s.type() for s in mb[0].main_path][-1] == "layer_scale"  # the first block: rate 0, no layer
    assert [n for n in names(m) if not n.startswith("drop_path")] == names(base)
    t = create_model("convnext_tiny_tiny_imagenet", drop_path_rate=0.1)
    dt = dps(t)
    assert len(dt) == 17 and dt[-1].drop_rate == pytest.approx(0.1) and dt[0].drop_rate == pytest.approx(0.1 / 17)
    with pytest.raises(ValueError):
        create_model("convnext_pico_cifar10", drop_path_rate=1.0)


def test_planner_drop_tail_rule():
    """RF_DROP_TAIL comes with RF_SCALE_TAIL for ... LayerScale, DropPath with an identity shortcut and
    no activation, and nowhere else; a DropPath behind a BatchNorm claims no fused tail."""
    from dcnn_amd.nn.layers.residual import fuse_kinds
    from dcnn_amd.ops._ext import kernels
    K = kernels()
    assert (K.FK_DROPPATH, K.RF_DROP_TAIL) == (10, 8)
    C, B, R, A, O, L, D = K.FK_CONV, K.FK_BN, K.FK_RELU, K.FK_ACT, K.FK_OTHER, K.FK_LSCALE, K.FK_DROPPATH
    kinds = fuse_kinds(_block_net(0.5, 1).layers[0].main_path)
    assert kinds == [O, O, C, A, C, L, D]
    both = K.RF_SCALE_TAIL | K.RF_DROP_TAIL
    assert K.plan_residual_fusions(kinds, [], True, True) == both
    assert K.plan_residual_fusions(kinds, [], True, False) == 0          # relu block
    assert K.plan_residual_fusions(kinds, [C, B], True, True) == 0       # projection shortcut
    assert K.plan_residual_fusions([C, D, L], [], True, True) == K.RF_SCALE_TAIL  # a DropPath elsewhere
    assert K.plan_residual_fusions([C, L, D, D], [], True, True) == 0
    assert K.plan_residual_fusions([L, D], [], True, True) == 0
    assert K.plan_residual_fusions(kinds[:-1], [], True, True) == K.RF_SCALE_TAIL  # as before
    assert K.plan_residual_fusions([C, B, R, C, B, D], [], True, False) == 0     # ResNet block + DropPath
    assert K.plan_residual_fusions([C, B, R, C, B], [], True, False) == K.RF_FUSED_TAIL
    assert K.plan_sequence_fusions([C, B, D]) == [K.FF_EMIT_BN_STATS, 0, 0]
