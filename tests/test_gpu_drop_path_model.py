"""DropPath at the model level on the GPU: two ConvNeXt blocks with stochastic depth take the drop tail
(the mask inside the LayerScale's residual store, no separate add, no standalone DropPath launch) and
match the CPU backend, which draws the same masks from the same seeds (teacher-forced bf16 with the
per-tensor bounds of tests/test_gpu_convnext_model.py, and the fp32 compute dtype); captured steps
equal eager steps bit for bit; a ResNet basic block with a DropPath behind its last BatchNorm takes
the plain path with the standalone kernels and matches the CPU too."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CL = torch.channels_last
N = 6


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def two_block_net():
    """3x16x16 input, 2x2 s2 stem -> 16 channels on an 8x8 map, two ConvNeXt blocks at rate 0.5 with
    explicit seeds, pool, dense. Layer scale 0.5: the branch must weigh in the block's output."""
    from dcnn_amd.nn import SequentialBuilder
    return (SequentialBuilder("cnx_dp").input([3, 16, 16])
            .conv2d(16, 2, 2, 2, 2, 0, 0, True, "stem_conv").layernorm(1e-6, True, "stem_ln")
            .convnext_block(16, 0.5, "block1", drop_path=0.5, drop_path_seed=101)
            .convnext_block(16, 0.5, "block2", drop_path=0.5, drop_path_seed=(1 << 40) + 7)
            .avgpool2d(8, 8, 1, 1, 0, 0, "avgpool").layernorm(1e-6, True, "head_ln").flatten("flatten")
            .dense(10, True, "fc").build())


def _pair(make, seed=3, dtype=None):
    cpu = make()
    cpu.set_seed(seed)
    cpu.initialize()
    gpu = make()
    gpu.set_seed(seed)
    gpu.set_device("GPU:0")
    if dtype is not None:
        gpu.set_compute_dtype(dtype)
    gpu.initialize()
    for a, b in zip(cpu.parameters(), gpu.parameters()):
        assert torch.equal(a, b.cpu())
    return cpu, gpu


def _blocks(m):
    return [l for l in m.layers if l.type() == "residual_block"]


def _teacher_forced(cpu, gpu, x, y, to_gpu=lambda t: t.cuda()):
    """Every GPU layer gets the bf16-emulated CPU layer's input and output gradient; each layer runs
    forward once on either side, so the DropPath draw indices agree. Bounds: 0.01 forward, 0.06 input
    gradient, 0.06 parameter gradients with the 0.05 x scale floor
    (tests/test_gpu_convnext_model.py::test_convnext_layers_teacher_forced)."""
    from dcnn_amd.nn import LossFactory
    cpu.clear_gradients()
    gpu.clear_gradients()
    acts, outs = [x], []
    for lc, lg in zip(cpu.layers, gpu.layers):
        acts.append(lc.forward(acts[-1]))
        outs.append(lg.forward(to_gpu(acts[-2])))
    for lg, out, ref in zip(gpu.layers, outs, acts[1:]):
        e = rel(out, ref)
        print(f"{lg.name}: fwd {e:.2e}")
        assert e < 0.01, (lg.name, e)
    _, g, _ = LossFactory.create("softmax_crossentropy").loss_and_grad(acts[-1], y)
    for lc, lg in zip(reversed(cpu.layers), reversed(gpu.layers)):
        dxg = lg.backward(to_gpu(g))
        g_in, g = g, lc.backward(g)
        if g is not None and dxg is not None:
            e = rel(dxg, g)
            print(f"{lg.name}: dx {e:.2e}")
            assert e < 0.06, (lg.name, e)
        gc = [a.reshape(-1) for a in lc.gradients()]
        gg = [b.float().cpu().reshape(-1) for b in lg.gradients()]
        if gc:
            scale = max(a.norm().item() for a in gc)
            for j, (a, b) in enumerate(zip(gc, gg)):
                e = (a - b).norm().item() / max(a.norm().item(), 0.05 * scale)
                print(f"{lg.name}: g{j} {e:.2e}")
                assert e < 0.06, (lg.name, j, e)


def _same_masks(cpu, gpu):
    both = False
    for bc, bg in zip(_blocks(cpu), _blocks(gpu)):
        mc, mg = bc.main_path[-1].last_mask(), bg.main_path[-1].last_mask().cpu()
        assert torch.equal(mc, mg)
        both = both or ((mc == 0).any().item() and (mc != 0).any().item())
    assert both, "the seeds drop some samples and keep others"


def test_two_blocks_bf16_teacher_forced():
    from test_gpu_convnext_model import bf16_emulate
    torch.manual_seed(0)
    x, y = torch.randn(N, 3, 16, 16), torch.randint(0, 10, (N,))
    cpu, gpu = _pair(two_block_net)
    assert [(b._scale_tail, b._drop_tail, b._fused) for b in _blocks(gpu)] == [(True, True, False)] * 2
    assert [(b._scale_tail, b._drop_tail) for b in _blocks(cpu)] == [(False, False)] * 2
    bf16_emulate(cpu)
    gpu.load_parameters([p.clone() for p in cpu.parameters()])
    _teacher_forced(cpu, gpu, x, y)
    _same_masks(cpu, gpu)


def test_drop_tail_launches():
    """One lscale_drop_fwd carrying residual and mask, one lscale_drop_bwd, the shortcut gradient in
    the depthwise data gradient's store: no separate add, no standalone DropPath launch."""
    from dcnn_amd.ops import hip
    torch.manual_seed(1)
    _, gpu = _pair(two_block_net)
    blk = _blocks(gpu)[0]
    x = torch.randn(N, 16, 8, 8).cuda()
    with hip.record_convs() as calls:
        y = blk.forward(x)
    ops = [c["op"] for c in calls]
    assert ops.count("lscale_drop_fwd") == 1 and ops.count("drop_path_mask") == 1
    assert "lscale_fwd" not in ops and "drop_path_scale" not in ops
    with hip.record_convs() as calls:
        dx = blk.backward(torch.randn_like(y))
    ops = [c["op"] for c in calls]
    assert ops.count("lscale_drop_bwd") == 1 and "lscale_bwd" not in ops and "drop_path_scale" not in ops
    dg = [c for c in calls if c["op"] == "dw_dgrad"]
    assert len(dg) == 1 and dg[0]["residual"] is True
    assert tuple(dx.shape) == (N, 16, 8, 8)
    # a dropped sample's output is its input (the branch weighs nothing), bit for bit
    m = blk.main_path[-1].last_mask().cpu()
    xa = hip.to_act(x, torch.bfloat16)
    for n in range(N):
        if m[n] == 0:
            assert torch.equal(y[n], xa[n])
    # eval mode: the DropPath is the identity and the block is the plain scale tail
    gpu.set_training(False)
    with hip.record_convs() as calls:
        blk.forward(x)
    ops = [c["op"] for c in calls]
    assert ops.count("lscale_fwd") == 1 and "lscale_drop_fwd" not in ops and "drop_path_mask" not in ops


def test_two_blocks_fp32_step_matches_cpu():
    """The exact fp32 compute dtype against the CPU float32 model: logits within 1e-4
    (tests/test_gpu_convnext_model.py::test_fp32_compute_dtype_matches_cpu), gradients within that
    file's per-tensor bound."""
    from dcnn_amd.nn import LossFactory
    torch.manual_seed(2)
    x, y = torch.randn(N, 3, 16, 16), torch.randint(0, 10, (N,))
    cpu, gpu = _pair(two_block_net, seed=1, dtype=torch.float32)
    assert all(b._drop_tail for b in _blocks(gpu))
    lf = LossFactory.create("softmax_crossentropy")
    yc = cpu.forward(x)
    yg = gpu.forward(x.cuda(), return_on_input_device=False)
    _same_masks(cpu, gpu)
    e = rel(yg, yc)
    print(f"fp32 logits rel err {e:.2e}")
    assert e < 1e-4, e
    _, gc, _ = lf.loss_and_grad(yc, y)
    cpu.clear_gradients()
    gpu.clear_gradients()
    cpu.backward(gc)
    gpu.backward(gc.cuda())
    torch.cuda.synchronize()
    gcs = [a.reshape(-1) for a in cpu.gradients()]
    ggs = [b.float().cpu().reshape(-1) for b in gpu.gradients()]
    scale = max(a.norm().item() for a in gcs)
    for j, (a, b) in enumerate(zip(gcs, ggs)):
        err = (a - b).norm().item() / max(a.norm().item(), 0.05 * scale)
        print(f"g{j} {err:.2e}")
        assert err < 0.06, (j, err)


def _train(make):
    from dcnn_amd.nn import AdamW, LossFactory
    m = make()
    m.set_seed(5)
    m.set_device("GPU:0")
    m.initialize()
    m.set_first_layer_input_grad(False)
    opt = AdamW(1e-3, weight_decay=0.05, no_decay_norm_bias=True)
    opt.attach(m)
    return m, opt, LossFactory.create("softmax_crossentropy")


def test_captured_steps_equal_eager_steps():
    from dcnn_amd.runtime.step import TrainStep
    torch.manual_seed(1)
    xs = [torch.randn(N, 3, 16, 16, device="cuda") for _ in range(3)]
    ys = [torch.randint(0, 10, (N,), device="cuda") for _ in range(3)]
    m, opt, lf = _train(two_block_net)
    m2, opt2, lf2 = _train(two_block_net)
    st, st2 = TrainStep(m, lf, opt, use_graph=False), TrainStep(m2, lf2, opt2, use_graph=True)
    masks = []
    for x, y in zip(xs, ys):
        st(x, y)
        st2(x, y)
        torch.cuda.synchronize()
        assert float(st.last_loss.item()) == float(st2.last_loss.item())
        for b, b2 in zip(_blocks(m), _blocks(m2)):
            assert torch.equal(b.main_path[-1].last_mask(), b2.main_path[-1].last_mask())
        masks.append(_blocks(m2)[0].main_path[-1].last_mask().cpu())
        assert torch.equal(m.arena.data, m2.arena.data)
    assert st2.graphs is not None and opt.t == opt2.t == 3
    from dcnn_amd.ops import cpu
    for k, mk in enumerate(masks):  # replay k drew index k + 1
        assert torch.equal(mk, cpu.drop_path_mask(101, k + 1, N, 0.5))


def resnet_block_net():
    """conv-BN-ReLU-conv-BN-DropPath, identity shortcut, ReLU; C = 16 on a 4x4 map."""
    from dcnn_amd.nn import SequentialBuilder
    from dcnn_amd.nn.layers import LayerBuilder
    main = (LayerBuilder().input([16, 4, 4])
            .conv2d(16, 3, 3, 1, 1, 1, 1, True).batchnorm(1e-5, 0.1, True, "bn0").activation("relu")
            .conv2d(16, 3, 3, 1, 1, 1, 1, True).batchnorm(1e-5, 0.1, True, "bn1")
            .drop_path(0.5, "dp", seed=77).build())
    return (SequentialBuilder("res_dp").input([16, 4, 4]).residual(main, [], "relu", "block")
            .flatten("flatten").dense(10, True, "fc").build())


def test_resnet_block_takes_the_plain_path():
    from dcnn_amd.nn.layers.residual import fuse_kinds
    from dcnn_amd.ops import hip
    from dcnn_amd.ops._ext import kernels
    from test_gpu_model import bf16_emulate
    torch.manual_seed(3)
    n = 4
    x = torch.randn(n, 16, 4, 4).bfloat16().float()
    y = torch.randint(0, 10, (n,))
    cpu, gpu = _pair(resnet_block_net)
    blk = gpu.layers[0]
    K = kernels()
    kinds = fuse_kinds(blk.main_path)
    assert kinds[-1] == K.FK_DROPPATH and K.plan_residual_fusions(kinds, [], True, False) == 0
    assert not blk._fused and not blk._scale_tail and not blk._drop_tail
    bf16_emulate(cpu)
    gpu.load_parameters([p.clone() for p in cpu.parameters()])
    with hip.record_convs() as calls:
        _teacher_forced(cpu, gpu, x, y, to_gpu=lambda t: hip.to_act(t.cuda(), torch.bfloat16) if t.dim() == 4 and
                        t.shape[2] > 1 else t.cuda())
    ops = [c["op"] for c in calls]
    assert ops.count("drop_path_scale") == 2 and ops.count("drop_path_mask") == 1  # forward and backward
    assert "lscale_drop_fwd" not in ops
    mc, mg = cpu.layers[0].main_path[-1].last_mask(), blk.main_path[-1].last_mask().cpu()
    assert torch.equal(mc, mg) and (mc == 0).any() and (mc != 0).any()
