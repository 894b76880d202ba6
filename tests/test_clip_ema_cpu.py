"""Global-norm gradient clipping (``max_grad_norm``) and the weight EMA (``ema_decay``) of the optimizer
step on the CPU: the native flat-buffer step of an arena (ops/cpu.py adam_step_tail / sgd_step_tail /
grad_sumsq / ema_swap) and the per-parameter fallback of nn/optimizers.py, against a float64
per-parameter formula written here (never the code under test).

Adam is nearly invariant to a constant gradient scale, so the gradients of the three steps are randn
times 1, 100 and 0.01: with ``max_grad_norm`` = 5 the first step clips, the second clips hard and the
third does not clip, and the moments mix all three. Every "matches the formula" test also asserts that
the result does NOT match the unclipped formula, and that the EMA moved."""
import math
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_decay_exclusion import EXPECTED, _model, _raw_arena

LR, B1, B2, EPS, WD, MOM = 0.01, 0.9, 0.999, 1e-8, 0.1, 0.9
MAXN, DECAY = 5.0, 0.9
SCALES = (1.0, 100.0, 0.01)
TOL = dict(atol=1e-6, rtol=1e-5)  # tests/test_training_components.py::test_optimizer_update_rules

# kind -> (constructor keyword arguments, decoupled, weight decay of parameter i)
KINDS = ["adam_l2", "adamw", "adamw_nodecay", "sgd_momentum"]
SWITCHES = {"clip": (MAXN, 0.0), "ema": (0.0, DECAY), "both": (MAXN, DECAY)}


def make_opt(kind, max_norm, decay):
    from dcnn_amd.nn import SGD, Adam
    if kind == "sgd_momentum":
        return SGD(LR, MOM, max_grad_norm=max_norm, ema_decay=decay)
    return Adam(LR, B1, B2, EPS, WD, kind != "adam_l2", no_decay_norm_bias=kind == "adamw_nodecay",
                max_grad_norm=max_norm, ema_decay=decay)


def reference(kind, p0, grads_per_step, no_decay, max_norm, decay):
    """float64, per parameter: the global norm over ALL gradients, coef = min(1, max / (norm + 1e-6)),
    the step on g * coef, then ema = d ema + (1 - d) p. Returns (params, ema, [(sumsq, norm, coef)])."""
    ref = [p.clone().double() for p in p0]
    ema = [r.clone() for r in ref]
    mm = [torch.zeros_like(r) for r in ref]
    vv = [torch.zeros_like(r) for r in ref]
    norms = []
    for t, grads in enumerate(grads_per_step, 1):
        grads = [g.double() for g in grads]
        sumsq = float(sum((g * g).sum() for g in grads))
        norm = math.sqrt(sumsq)
        coef = min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0
        norms.append((sumsq, norm, coef))
        bc1, bc2 = 1 - B1 ** t, 1 - B2 ** t
        for i, g in enumerate(grads):
            g = g * coef
            if kind == "sgd_momentum":
                mm[i] = MOM * mm[i] - LR * g
                ref[i] = ref[i] + mm[i]
            else:
                mm[i] = B1 * mm[i] + (1 - B1) * g
                vv[i] = B2 * vv[i] + (1 - B2) * g * g
                upd = LR * (mm[i] / bc1) / ((vv[i] / bc2).sqrt() + EPS)
                wd = 0.0 if (kind == "adamw_nodecay" and no_decay[i]) else WD
                if kind == "adam_l2":
                    upd = upd + wd * LR * ref[i]
                else:
                    ref[i] = ref[i] - wd * LR * ref[i]
                ref[i] = ref[i] - upd
            if decay > 0:
                ema[i] = decay * ema[i] + (1 - decay) * ref[i]
    return ref, ema, norms


def set_grads(grad_tensors, step):
    """randn times SCALES[step - 1] into the given gradient tensors; returns CPU copies"""
    g = torch.Generator().manual_seed(100 + step)
    out = []
    for gr in grad_tensors:
        v = torch.randn(gr.shape, generator=g) * SCALES[step - 1]
        gr.copy_(v.to(gr.device))
        out.append(v)
    return out


def check_run(kind, sw, params, grad_tensors, opt, p0, no_decay, ema_views, sync=lambda: None):
    """Three steps; parameters, EMA and the norm scalars after EACH step against the formula."""
    max_norm, decay = SWITCHES[sw]
    per_step = []
    for s in (1, 2, 3):
        per_step.append(set_grads(grad_tensors, s))
        before = [g.detach().cpu().clone() for g in grad_tensors]
        opt.update()
        sync()
        # the gradient buffers are not rewritten: model.gradients() still shows the unclipped gradient
        assert all(torch.equal(a, g.detach().cpu()) for a, g in zip(before, grad_tensors))
        if max_norm > 0:
            _, _, norms = reference(kind, p0, per_step, no_decay, max_norm, decay)
            blk = opt.grad_norm_device.detach().cpu().double()
            want = torch.tensor([*norms[-1], max_norm], dtype=torch.float64)
            assert torch.allclose(blk, want, rtol=1e-5, atol=0), (s, blk, want)
            assert opt.last_grad_norm() == pytest.approx(norms[-1][1], rel=1e-5)
    ref, ema, norms = reference(kind, p0, per_step, no_decay, max_norm, decay)
    for i, (p, r) in enumerate(zip(params, ref)):
        assert torch.allclose(p.detach().cpu(), r.float(), **TOL), (i, "params")
    if max_norm > 0:
        assert norms[0][2] < 1 and norms[1][2] < 0.01 and norms[2][2] == 1.0  # clips, clips hard, does not clip
        unclipped, _, _ = reference(kind, p0, per_step, no_decay, 0.0, decay)
        assert not all(torch.allclose(p.detach().cpu(), r.float(), **TOL) for p, r in zip(params, unclipped))
    else:
        assert opt.grad_norm_device is None and opt.last_grad_norm() is None
    if decay > 0:
        for i, (e, r) in enumerate(zip(ema_views(), ema)):
            assert torch.allclose(e.detach().cpu(), r.float(), **TOL), (i, "ema")
        # the no-EMA outcomes: the average neither stayed at the initial weights nor equals the live ones
        assert not all(torch.allclose(e.detach().cpu(), p, **TOL) for e, p in zip(ema_views(), p0))
        assert not all(torch.allclose(e.detach().cpu(), p.detach().cpu(), **TOL) for e, p in zip(ema_views(), params))
    else:
        assert opt.ema is None
    return per_step


def model_case(kind, sw, device=None):
    m = _model(device)
    sync = torch.cuda.synchronize if device is not None else (lambda: None)
    p0 = [p.detach().cpu().clone() for p in m.parameters()]
    opt = make_opt(kind, *SWITCHES[sw])
    opt.attach(m)
    assert opt.arena is m.arena
    if SWITCHES[sw][1] > 0:
        assert len(opt.ema) == 1 and torch.equal(opt.ema[0], m.arena.data)  # a copy of the weights at attach
    views = lambda: [m.arena._view(opt.ema[0], i) for i in range(len(p0))]  # noqa: E731
    check_run(kind, sw, m.parameters(), m.gradients(), opt, p0, EXPECTED, views, sync)
    return m, opt


def raw_case(kind, sw, device="cpu"):
    ar = _raw_arena(device)
    sync = torch.cuda.synchronize if str(device) != "cpu" else (lambda: None)
    p0 = [ar.param(i).detach().cpu().clone() for i in range(3)]
    opt = make_opt(kind, *SWITCHES[sw])
    opt.attach([ar.param(i) for i in range(3)], [ar.grad_view(i) for i in range(3)], ar)
    assert opt.arena is ar
    views = lambda: [ar._view(opt.ema[0], i) for i in range(3)]  # noqa: E731
    check_run(kind, sw, [ar.param(i) for i in range(3)], [ar.grad_view(i) for i in range(3)], opt, p0,
              [False, True, False], views, sync)
    # the padding between the slices (elements 70..127, 200..255) stays zero, in data and in ema
    for buf in [ar.data] + ([opt.ema[0]] if opt.ema else []):
        flat = buf.cpu()
        assert (flat[70:128] == 0).all() and (flat[200:] == 0).all()


@pytest.mark.parametrize("sw", list(SWITCHES))
@pytest.mark.parametrize("kind", KINDS)
def test_three_steps_match_the_formula_model(kind, sw):
    model_case(kind, sw)


@pytest.mark.parametrize("sw", list(SWITCHES))
@pytest.mark.parametrize("kind", KINDS)
def test_three_steps_match_the_formula_raw_arena(kind, sw):
    raw_case(kind, sw)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_native_grad_sumsq(dtype):
    from dcnn_amd.ops import cpu
    for n in (1, 3, 64, 4099, 70001):
        g = torch.randn(n, generator=torch.Generator().manual_seed(n), dtype=dtype) * 3
        assert cpu.grad_sumsq(g) == pytest.approx(float((g.double() ** 2).sum()), rel=1e-12)


@pytest.mark.parametrize("kind", KINDS)
def test_per_parameter_fallback(kind):
    """No arena: plain tensors. The norm is taken over all parameters, not per tensor."""
    m = _model()
    p0 = [p.detach().clone() for p in m.parameters()]
    params = [p.clone() for p in p0]
    grads = [torch.zeros_like(p) for p in p0]
    opt = make_opt(kind, MAXN, DECAY)
    opt.attach(params, grads, no_decay=EXPECTED)
    assert opt.arena is None and len(opt.ema) == len(params)
    check_run(kind, "both", params, grads, opt, p0, EXPECTED, lambda: opt.ema)


@pytest.mark.parametrize("kind", ["adamw", "sgd_momentum"])
def test_zero_gradient(kind):
    m = _model()
    p0 = [p.detach().clone() for p in m.parameters()]
    opt = make_opt(kind, MAXN, DECAY)
    opt.attach(m)
    opt.clear_gradients()
    opt.update()
    assert opt.grad_norm_device.tolist() == [0.0, 0.0, 1.0, MAXN]
    assert torch.isfinite(m.arena.data).all() and torch.isfinite(opt.ema[0]).all()
    if kind == "sgd_momentum":
        assert all(torch.equal(p, q) for p, q in zip(m.parameters(), p0))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("arena", [True, False], ids=["arena", "per_parameter"])
def test_huge_max_norm_is_bit_identical_to_the_plain_step(kind, arena):
    """max_grad_norm = 1e30: coef is exactly 1, and g * 1 through the same step gives the same bits."""
    def run(max_norm):
        m = _model()
        opt = make_opt(kind, max_norm, 0.0)
        if arena:
            opt.attach(m)
            params, grads = m.parameters(), m.gradients()
        else:
            params = [p.detach().clone() for p in m.parameters()]
            grads = [torch.zeros_like(p) for p in params]
            opt.attach(params, grads, no_decay=EXPECTED)
        for s in (1, 2, 3):
            set_grads(grads, s)
            opt.update()
        return params, opt
    a, oa = run(1e30)
    b, _ = run(0.0)
    assert oa.grad_norm_device[2].item() == 1.0
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("kind", ["adamw_nodecay", "sgd_momentum"])
def test_switches_off_take_the_old_launch_path(kind, monkeypatch):
    from dcnn_amd.ops import cpu

    def boom(*a, **k):
        raise AssertionError("the tail entry point was reached with both switches off")
    for name in ("adam_step_tail", "sgd_step_tail", "grad_sumsq", "ema_swap"):
        monkeypatch.setattr(cpu, name, boom)
    m = _model()
    opt = make_opt(kind, 0.0, 0.0)
    opt.attach(m)
    set_grads(m.gradients(), 1)
    opt.update()
    with opt.ema_weights():  # no-op when the EMA is off
        pass
    assert opt.ema is None and opt.grad_norm_device is None and "ema" not in opt.state_dict()
    # and with a switch on the tail entry point IS the path
    opt2 = make_opt(kind, MAXN, 0.0)
    opt2.attach(_model())
    with pytest.raises(AssertionError, match="tail entry point"):
        opt2.update()


def test_config_factory_clone_and_range_errors():
    from dcnn_amd.nn import SGD, Adam, AdamW, OptimizerFactory
    for o in (Adam(), AdamW(), SGD()):
        assert o.max_grad_norm == 0.0 and o.ema_decay == 0.0
    for o in (AdamW(0.002, weight_decay=0.05, max_grad_norm=2.5, ema_decay=0.999),
              Adam(0.002, max_grad_norm=2.5, ema_decay=0.999), SGD(0.1, 0.9, max_grad_norm=2.5, ema_decay=0.999)):
        cfg = o.get_config()
        assert cfg["parameters"]["max_grad_norm"] == 2.5 and cfg["parameters"]["ema_decay"] == 0.999
        for o2 in (OptimizerFactory.create_from_config(cfg.to_json()), o.clone()):
            assert type(o2) in (Adam, SGD) and o2.max_grad_norm == 2.5 and o2.ema_decay == 0.999
            assert o2.get_config()["type"] == cfg["type"]
    for old in ({"type": "adamw", "parameters": {"learning_rate": 0.004, "weight_decay": 0.02}},
                {"type": "sgd", "parameters": {"learning_rate": 0.1}}):
        o = OptimizerFactory.create_from_config(old)
        assert o.max_grad_norm == 0.0 and o.ema_decay == 0.0
    for cls in (Adam, AdamW, SGD):
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="max_grad_norm"):
                cls(max_grad_norm=bad)
        for bad in (-0.1, 1.0, 1.5, float("nan")):
            with pytest.raises(ValueError, match="ema_decay"):
                cls(ema_decay=bad)


def test_training_config_fields(monkeypatch):
    from dcnn_amd.nn import AdamW
    from dcnn_amd.nn.train import TrainingConfig, apply_step_options
    assert TrainingConfig().max_grad_norm == 0.0 and TrainingConfig().ema_decay == 0.0
    monkeypatch.setenv("MAX_GRAD_NORM", "5.0")
    monkeypatch.setenv("EMA_DECAY", "0.9999")
    cfg = TrainingConfig().load_from_env()
    assert cfg.max_grad_norm == 5.0 and cfg.ema_decay == 0.9999
    opt = AdamW()
    apply_step_options(opt, cfg)
    assert opt.max_grad_norm == 5.0 and opt.ema_decay == 0.9999
    cfg.ema_decay = 1.0
    with pytest.raises(ValueError, match="ema_decay"):
        apply_step_options(AdamW(), cfg)


def test_ema_weights_context():
    m, opt = model_case("adamw", "both")
    data, ema, shadow = m.arena.data.clone(), opt.ema[0].clone(), None
    if m.arena.shadow is not None:
        shadow = m.arena.shadow.clone()
    assert not torch.equal(data, ema)
    with opt.ema_weights():
        assert torch.equal(m.arena.data, ema) and torch.equal(opt.ema[0], data)
        assert all(torch.equal(p, m.arena._view(ema, i)) for i, p in enumerate(m.parameters()))
    assert torch.equal(m.arena.data, data) and torch.equal(opt.ema[0], ema)
    if shadow is not None:
        assert torch.equal(m.arena.shadow, shadow)
    with pytest.raises(RuntimeError):  # an exception inside still swaps back
        with opt.ema_weights():
            raise RuntimeError("x")
    assert torch.equal(m.arena.data, data) and torch.equal(opt.ema[0], ema)


def test_validation_runs_on_the_ema_weights():
    """train.py validates inside ema_weights(): the forward there is the forward of a model whose
    weights are the EMA (the BatchNorm running statistics stay the live ones)."""
    m, opt = model_case("adamw", "ema")
    m.set_training(False)
    x = torch.randn(2, 4, 6, 6, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        live = m.forward(x).clone()
        with opt.ema_weights():
            avg = m.forward(x).clone()
    m2 = _model()
    m2.arena.data.copy_(opt.ema[0])
    m2.arena.sync_shadow(force=True)
    from dcnn_amd.parallel.dp import _bn_buffers
    for la, lb in zip(m.layers, m2.layers):
        for a, b in zip(_bn_buffers(la), _bn_buffers(lb)):
            b.copy_(a)
    m2.set_training(False)
    with torch.no_grad():
        want = m2.forward(x)
    assert torch.equal(avg, want) and not torch.equal(avg, live)


def test_checkpoint_carries_the_ema(tmp_path):
    from dcnn_amd.nn.train import load_checkpoint, save_checkpoint
    m, opt = model_case("adamw", "both")
    path = str(tmp_path / "ckpt")
    save_checkpoint(m, opt, path, epoch=3)
    m2 = _model()
    opt2 = make_opt("adamw", MAXN, DECAY)
    assert load_checkpoint(m2, opt2, path) == 3
    assert torch.equal(opt2.ema[0], opt.ema[0]) and not torch.equal(opt2.ema[0], m2.arena.data)
    assert torch.equal(m2.arena.data, m.arena.data) and opt2.t == opt.t


def test_pipeline_stage_refuses_the_switches():
    from dcnn_amd.nn import SGD, AdamW
    from dcnn_amd.parallel.pipeline.config import StageConfig
    from dcnn_amd.parallel.pipeline.stage import PipelineStage

    class _Comm:
        id = "stage_0"

        def send(self, m):
            pass

    m = _model()
    for opt, key in ((AdamW(max_grad_norm=1.0), "max_grad_norm"), (SGD(ema_decay=0.5), "ema_decay")):
        cfg = StageConfig("stage_0", 0, 1, m.get_config(), dict(opt.get_config()))
        st = PipelineStage(_Comm())
        with pytest.raises(ValueError, match=key):
            st._configure(cfg.dumps())
        assert st.optimizer is None
    cfg = StageConfig("stage_0", 0, 1, m.get_config(), dict(AdamW().get_config()))
    st = PipelineStage(_Comm())
    st._configure(cfg.dumps())  # both off: accepted
    assert st.optimizer is not None


# ------------------------------------------------------------------------------- data parallel
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


DP_MAX = 0.05


def _dp_model(seed):
    """no BatchNorm: two half-batches then compute exactly what the whole batch computes"""
    from dcnn_amd.nn import SequentialBuilder
    m = (SequentialBuilder("dp_clip").input([3, 8, 8]).conv2d(8, 3, 3, 1, 1, 1, 1, True, "conv")
         .layernorm(1e-6, True, "ln").activation("relu", "relu").flatten("flatten").dense(10, True, "fc").build())
    m.set_seed(seed)
    m.initialize()
    return m


def _dp_batch():
    g = torch.Generator().manual_seed(7)
    return torch.randn(8, 3, 8, 8, generator=g), torch.randint(0, 10, (8,), generator=g)


def _dp_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from dcnn_amd.nn import SGD, LossFactory
    from dcnn_amd.parallel.dp import DataParallel
    from dcnn_amd.runtime.step import TrainStep
    model = _dp_model(100 + rank)  # different init per rank: the broadcast unifies it
    dp = DataParallel(model, bucket_mb=0.001)
    opt = SGD(0.05, MOM, max_grad_norm=DP_MAX, ema_decay=DECAY)
    opt.attach(model)
    step = TrainStep(dp, LossFactory.create("softmax_crossentropy"), opt)
    x, y = _dp_batch()
    step(x[rank * 4:(rank + 1) * 4], y[rank * 4:(rank + 1) * 4])
    torch.save({"params": [p.detach().clone() for p in model.parameters()], "norm": opt.grad_norm_device.clone(),
                "ema": opt.ema[0].clone(), "nbuckets": len(dp.buckets)}, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_dp_clips_the_averaged_gradient(tmp_path):
    """World size 2 over gloo: the clipped step on two half-batches equals the single-process clipped
    step on the whole batch, so the norm is taken after the all-reduce mean (a per-rank norm taken
    before it would give another coefficient)."""
    mp.spawn(_dp_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0 = torch.load(tmp_path / "rank0.pt", weights_only=True)
    r1 = torch.load(tmp_path / "rank1.pt", weights_only=True)
    assert r0["nbuckets"] > 1
    for a, b in zip(r0["params"], r1["params"]):
        assert torch.equal(a, b)
    assert torch.equal(r0["norm"], r1["norm"])
    from dcnn_amd.nn import SGD, LossFactory
    ref = _dp_model(100)
    p0 = [p.detach().clone() for p in ref.parameters()]
    opt = SGD(0.05, MOM, max_grad_norm=DP_MAX, ema_decay=DECAY)
    opt.attach(ref)
    x, y = _dp_batch()
    opt.clear_gradients()
    _, grad, _ = LossFactory.create("softmax_crossentropy").loss_and_grad(ref.forward(x), y)
    ref.backward(grad)
    opt.update()
    coef = opt.grad_norm_device[2].item()
    assert coef < 0.5  # the clip is active, so its placement matters
    assert torch.allclose(r0["norm"], opt.grad_norm_device, rtol=1e-5, atol=0)
    for a, b in zip(r0["params"], ref.parameters()):
        assert torch.allclose(a, b, **TOL)
    assert torch.allclose(r0["ema"], opt.ema[0], **TOL)
    # a rank-local norm differs: the half-batch gradients are not the averaged gradient
    lf = LossFactory.create("softmax_crossentropy")
    half = _dp_model(100)
    half.clear_gradients()
    _, g0, _ = lf.loss_and_grad(half.forward(x[:4]), y[:4])
    half.backward(g0)
    local = math.sqrt(sum(float((g.double() ** 2).sum()) for g in half.gradients()))
    assert abs(local - r0["norm"][1].item()) / r0["norm"][1].item() > 1e-3
    # and an unclipped step lands elsewhere
    un = [p - 0.05 * g for p, g in zip(p0, ref.gradients())]
    assert not all(torch.allclose(a, b, **TOL) for a, b in zip(r0["params"], un))
