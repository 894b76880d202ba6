"""AdamW / Adam with biases, norm affines and layer scales excluded from weight decay
(``no_decay_norm_bias``): the classification each layer makes of its own parameters, the step against
the per-parameter formula of nn/optimizers.py, the bit-identity guarantees (everything flagged ==
wd 0; switch off == the step as it was), the raw arena block table, and on the GPU the fused arena
kernel, eager and under the captured step."""
import pytest
import torch

LR, B1, B2, EPS, WD = 0.01, 0.9, 0.999, 1e-8, 0.1
TOL = dict(atol=1e-6, rtol=1e-5)  # tests/test_training_components.py::test_optimizer_update_rules


def _model(device=None):
    """conv with bias, BatchNorm, LayerNorm, LayerScale, a dense layer with ONE output (its weight
    has a bias's shape [1, F]: the classification must not go by shape)."""
    from dcnn_amd.nn import SequentialBuilder
    m = (SequentialBuilder("decay").input([4, 6, 6])
         .conv2d(8, 3, 3, 1, 1, 1, 1, True, "conv").batchnorm(1e-5, 0.1, True, "bn").layernorm(1e-6, True, "ln")
         .layer_scale(0.5, "ls").flatten("flatten").dense(1, True, "fc").build())
    m.set_seed(12)
    if device is not None:
        m.set_device(device)
        m.set_compute_dtype(torch.float32)
    m.initialize()
    return m


EXPECTED = [False, True, True, True, True, True, True, False, True]  # conv w b, bn g b, ln g b, ls g, fc w b


def _set_grads(m, step):
    g = torch.Generator().manual_seed(100 + step)
    for gr in m.gradients():
        gr.copy_(torch.randn(gr.shape, generator=g).to(gr.device))


def _formula(p0, grads_per_step, wd_of, decoupled):
    """The per-parameter loop of Adam.update (nn/optimizers.py), wd per parameter."""
    ref = [p.clone().double() for p in p0]
    mm = [torch.zeros_like(r) for r in ref]
    vv = [torch.zeros_like(r) for r in ref]
    for t, grads in enumerate(grads_per_step, 1):
        bc1, bc2 = 1 - B1 ** t, 1 - B2 ** t
        for i, g in enumerate(grads):
            g = g.double()
            mm[i] = B1 * mm[i] + (1 - B1) * g
            vv[i] = B2 * vv[i] + (1 - B2) * g * g
            upd = LR * (mm[i] / bc1) / ((vv[i] / bc2).sqrt() + EPS)
            wd = wd_of(i)
            if wd > 0:
                if decoupled:
                    ref[i] = ref[i] - wd * LR * ref[i]
                else:
                    upd = upd + wd * LR * ref[i]
            ref[i] = ref[i] - upd
    return ref


def _run(m, opt, steps=3):
    opt.attach(m)
    grads = []
    for s in range(1, steps + 1):
        _set_grads(m, s)
        grads.append([g.detach().cpu().clone() for g in m.gradients()])
        opt.update()
    if m.device.is_gpu():
        torch.cuda.synchronize()
    return grads


def test_classification():
    m = _model()
    assert m.no_decay_flags() == EXPECTED
    assert m.arena.no_decay_flags() == EXPECTED
    fc_w = m.parameters()[7]
    assert tuple(fc_w.shape)[0] == 1 and not m.no_decay_flags()[7]
    from dcnn_amd.nn.layers import DepthwiseConv2D, GroupNorm, GroupedConv2D
    for l, want in ((DepthwiseConv2D(8, 3, 3, 1, 1, 1, 1, True), [False, True]),
                    (GroupedConv2D(8, 8, 3, 3, 2, 1, 1, 1, 1, True), [False, True]),
                    (GroupNorm(2, 8), [True, True])):
        assert [s.no_decay for s in l.param_specs()] == want
    blocks = m.arena.no_decay_blocks()
    assert blocks.dtype == torch.uint8 and blocks.numel() == m.arena.numel // 64
    ends = m.arena.offsets[1:] + [m.arena.numel]
    for f, lo, hi in zip(EXPECTED, m.arena.offsets, ends):
        assert lo % 64 == 0 and bool(blocks[lo // 64:hi // 64].all()) == f and bool(blocks[lo // 64:hi // 64].any()) == f


@pytest.mark.parametrize("decoupled", [True, False], ids=["adamw", "adam_l2"])
def test_three_steps_match_the_formula_cpu(decoupled):
    from dcnn_amd.nn import Adam
    m = _model()
    p0 = [p.clone() for p in m.parameters()]
    opt = Adam(LR, B1, B2, EPS, WD, decoupled, no_decay_norm_bias=True)
    grads = _run(m, opt)
    assert opt._nodecay_blocks is not None  # the native flat-buffer step with the block table
    ref = _formula(p0, grads, lambda i: 0.0 if EXPECTED[i] else WD, decoupled)
    for i, (p, r) in enumerate(zip(m.parameters(), ref)):
        assert torch.allclose(p, r.float(), **TOL), i
    # and the exclusion matters: decaying everything moves the flagged parameters elsewhere
    full = _formula(p0, grads, lambda i: WD, decoupled)
    assert not torch.allclose(m.parameters()[2], full[2].float(), **TOL)


def test_per_parameter_fallback_honours_the_switch():
    from dcnn_amd.nn import AdamW
    m = _model()
    p0 = [p.clone() for p in m.parameters()]
    params = [p.clone() for p in p0]
    grads = [torch.zeros_like(p) for p in p0]
    opt = AdamW(LR, B1, B2, EPS, WD, no_decay_norm_bias=True)
    with pytest.raises(ValueError):
        opt.attach(params, grads)  # no model, no arena, no flags: nothing to go by
    opt.attach(params, grads, no_decay=EXPECTED)
    assert opt.arena is None
    per_step = []
    for s in range(1, 4):
        g = torch.Generator().manual_seed(100 + s)
        for gr in grads:
            gr.copy_(torch.randn(gr.shape, generator=g))
        per_step.append([x.clone() for x in grads])
        opt.update()
    ref = _formula(p0, per_step, lambda i: 0.0 if EXPECTED[i] else WD, True)
    for i, (p, r) in enumerate(zip(params, ref)):
        assert torch.allclose(p, r.float(), **TOL), i


def _flagged_only_model(device=None):
    """every parameter of a flagged kind: norm affines and a layer scale"""
    from dcnn_amd.nn import SequentialBuilder
    m = (SequentialBuilder("flagged").input([8, 3, 3]).batchnorm(1e-5, 0.1, True, "bn").layernorm(1e-6, True, "ln")
         .layer_scale(0.5, "ls").build())
    m.set_seed(2)
    if device is not None:
        m.set_device(device)
        m.set_compute_dtype(torch.float32)
    m.initialize()
    return m


def _bit_identity(device):
    from dcnn_amd.nn import AdamW
    a, b = _flagged_only_model(device), _flagged_only_model(device)
    assert all(a.no_decay_flags())
    _run(a, AdamW(LR, B1, B2, EPS, WD, no_decay_norm_bias=True))
    _run(b, AdamW(LR, B1, B2, EPS, 0.0))
    assert torch.equal(a.arena.data, b.arena.data)  # everything excluded == no decay at all
    c, d = _model(device), _model(device)
    oc = AdamW(LR, B1, B2, EPS, WD, no_decay_norm_bias=False)
    _run(c, oc)
    assert oc._nodecay_blocks is None
    # the step as it was: the plain adam_step over the same flat buffers
    d_opt = AdamW(LR, B1, B2, EPS, WD)
    d_opt.attach(d)
    mm, vv = d.arena.new_zeros(), d.arena.new_zeros()
    hyper = None if device is None else torch.tensor([LR, 0.0, 0.0, 0.0], device="cuda")
    for s in range(1, 4):
        _set_grads(d, s)
        args = (LR, B1, B2, EPS, 1 - B1 ** s, 1 - B2 ** s, WD, True)
        if device is None:
            from dcnn_amd.ops import cpu
            cpu.adam_step(d.arena.data, d.arena.grad, mm, vv, *args)
        else:  # the device-side step scalars, then adam_kernel, as Adam.launch_step issues them
            from dcnn_amd.ops import hip
            from dcnn_amd.ops._ext import kernels, stream_ptr
            kernels().adam_scalars(hyper.data_ptr(), B1, B2, stream_ptr())
            hip.adam_step(d.arena.data, d.arena.grad, mm, vv, None, *args, hyper)
    assert torch.equal(c.arena.data, d.arena.data)


def test_bit_identity_cpu():
    _bit_identity(None)


def _raw_arena(device):
    from dcnn_amd.nn.params import ParamArena, ParamSpec
    specs = [ParamSpec("a", (70,)), ParamSpec("b", (64,), no_decay=True), ParamSpec("c", (8,))]
    ar = ParamArena(specs, torch.device(device))
    assert ar.offsets == [0, 128, 192] and ar.numel == 256
    assert ar.no_decay_blocks().cpu().tolist() == [0, 0, 1, 0]
    g = torch.Generator().manual_seed(7)
    for i in range(3):
        ar.param(i).copy_(torch.randn(specs[i].shape, generator=g))
    return ar


def _raw_case(device):
    from dcnn_amd.nn import AdamW
    ar = _raw_arena(device)
    p0 = [ar.param(i).detach().cpu().clone() for i in range(3)]
    opt = AdamW(LR, B1, B2, EPS, WD, no_decay_norm_bias=True)
    opt.attach([ar.param(i) for i in range(3)], [ar.grad_view(i) for i in range(3)], ar)
    assert opt.arena is ar and opt.no_decay == [False, True, False]
    per_step = []
    g = torch.Generator().manual_seed(8)
    for _ in range(3):
        gs = [torch.randn(p.shape, generator=g) for p in p0]
        for i in range(3):
            ar.grad_view(i).copy_(gs[i])
        per_step.append(gs)
        opt.update()
    ref = _formula(p0, per_step, lambda i: 0.0 if i == 1 else WD, True)
    for i in range(3):
        assert torch.allclose(ar.param(i).cpu(), ref[i].float(), **TOL), i
    decayed = _formula(p0, per_step, lambda i: WD, True)
    assert not torch.allclose(ar.param(1).cpu(), decayed[1].float(), **TOL)
    # the padding between the slices (elements 70..127, 200..255) stays zero
    flat = ar.data.cpu()
    assert (flat[70:128] == 0).all() and (flat[200:] == 0).all()


def test_raw_arena_cpu():
    _raw_case("cpu")


def test_config_and_factory_carry_the_switch():
    from dcnn_amd.nn import Adam, AdamW, OptimizerFactory
    assert Adam().no_decay_norm_bias is False and AdamW().no_decay_norm_bias is False
    o = AdamW(0.002, weight_decay=0.05, no_decay_norm_bias=True)
    cfg = o.get_config()
    assert cfg["parameters"]["no_decay_norm_bias"] is True
    o2 = OptimizerFactory.create_from_config(cfg.to_json())
    assert o2.no_decay_norm_bias is True and o2.decouple_weight_decay and o2.weight_decay == 0.05
    assert o.clone().no_decay_norm_bias is True
    old = {"type": "adamw", "parameters": {"learning_rate": 0.004, "weight_decay": 0.02}}
    assert OptimizerFactory.create_from_config(old).no_decay_norm_bias is False


# ------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("decoupled", [True, False], ids=["adamw", "adam_l2"])
def test_three_steps_match_the_formula_gpu(decoupled):
    from dcnn_amd.nn import Adam
    m = _model("GPU:0")
    p0 = [p.detach().cpu().clone() for p in m.parameters()]
    opt = Adam(LR, B1, B2, EPS, WD, decoupled, no_decay_norm_bias=True)
    grads = _run(m, opt)
    assert opt.fused() and opt._nodecay_blocks.is_cuda
    ref = _formula(p0, grads, lambda i: 0.0 if EXPECTED[i] else WD, decoupled)
    for i, (p, r) in enumerate(zip(m.parameters(), ref)):
        assert torch.allclose(p.cpu(), r.float(), **TOL), i


@pytest.mark.gpu
def test_bit_identity_gpu():
    _bit_identity("GPU:0")


@pytest.mark.gpu
def test_raw_arena_gpu():
    _raw_case("cuda:0")


def _train_net():
    from dcnn_amd.nn import AdamW, LossFactory, SequentialBuilder
    m = (SequentialBuilder("decay_train").input([3, 16, 16])
         .conv2d(16, 2, 2, 2, 2, 0, 0, True, "stem_conv").layernorm(1e-6, True, "stem_ln")
         .convnext_block(16, 0.5, "block1")
         .avgpool2d(8, 8, 1, 1, 0, 0, "avgpool").layernorm(1e-6, True, "head_ln").flatten("flatten")
         .dense(10, True, "fc").build())
    m.set_seed(9)
    m.set_device("GPU:0")
    m.initialize()
    m.set_first_layer_input_grad(False)
    opt = AdamW(1e-3, weight_decay=WD, no_decay_norm_bias=True)
    opt.attach(m)
    return m, opt, LossFactory.create("softmax_crossentropy")


@pytest.mark.gpu
def test_captured_step_matches_eager():
    """Three replays of the captured step (the static block table inside the graph) leave the same
    bits as three eager steps."""
    from dcnn_amd.runtime.step import TrainStep
    torch.manual_seed(3)
    xs = [torch.randn(8, 3, 16, 16, device="cuda") for _ in range(3)]
    ys = [torch.randint(0, 10, (8,), device="cuda") for _ in range(3)]
    m, opt, lf = _train_net()
    st = TrainStep(m, lf, opt, use_graph=False)
    m2, opt2, lf2 = _train_net()
    st2 = TrainStep(m2, lf2, opt2, use_graph=True)
    for x, y in zip(xs, ys):
        st(x, y)
        st2(x, y)
    torch.cuda.synchronize()
    assert st2.graphs is not None and opt.t == opt2.t == 3
    assert torch.equal(m.arena.data, m2.arena.data)
    # and the excluded parameters did take the undecayed step: a fully decayed run differs
    m3, _, lf3 = _train_net()
    from dcnn_amd.nn import AdamW
    opt3 = AdamW(1e-3, weight_decay=WD)
    opt3.attach(m3)
    st3 = TrainStep(m3, lf3, opt3, use_graph=False)
    for x, y in zip(xs, ys):
        st3(x, y)
    torch.cuda.synchronize()
    assert not torch.equal(m.arena.data, m3.arena.data)
