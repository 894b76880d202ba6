"""Global-norm gradient clipping and the weight EMA on the GPU: the raw kernels of loss_optim.hip
(grad_sumsq, adam_tail_kernel, sgd_tail_kernel, ema_swap) against float64 formulas, the three-step
formula tests of tests/test_clip_ema_cpu.py on GPU:0, and the captured step against eager steps.

Sizes: 1 and 3 (no float4 at all: the scalar tail only), 64 and 4099 (one workgroup of 1024 lanes, no
ticket; 4099 with a scalar tail), 4160 (two workgroups through the ticket, the second ragged), 2**20 + 64
(257 workgroups through the ticket, a ragged last one), and 2**20 + 67 (the same with a scalar tail).

grad_sumsq against float64 at rtol 1e-5: a lane adds at most 61 terms in sequence (60 float4 loads and
the tail; one or two at these sizes), the last workgroup's lanes at most ceil(blocks / 256) <= 2, and the
trees are 2 + 6 + 4 levels (lane, wave, workgroup) and 8 levels (final), 20 in all: under
(64 + 20 + 2) 2^-24 ~ 5e-6 on the sum, half that on the norm."""
import pytest
import torch

from test_clip_ema_cpu import (B1, B2, DECAY, EPS, KINDS, LR, MAXN, MOM, SWITCHES, TOL, WD, make_opt, model_case,
                               raw_case, set_grads)
from test_decay_exclusion import _model, _train_net

pytestmark = pytest.mark.gpu
SIZES = [1, 3, 64, 4099, 4160, 2 ** 20 + 64, 2 ** 20 + 67]


def _randn(n, seed, scale=1.0):
    return (torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale).cuda()


@pytest.mark.parametrize("n", SIZES)
def test_grad_sumsq(n):
    from dcnn_amd.ops import hip
    g = _randn(n, n, 3.0)
    want = float((g.double() ** 2).sum())
    norm = want ** 0.5
    outs = [torch.full((4,), -1.0, device="cuda") for _ in range(2)]
    for o in outs:  # twice in a row on one stream, eager: the ticket word resets itself
        hip.grad_sumsq(g, 2.0, o)
    torch.cuda.synchronize()
    ref = torch.tensor([want, norm, min(1.0, 2.0 / (norm + 1e-6)), 2.0], dtype=torch.float64)
    print(n, outs[0].tolist(), ref.tolist())
    assert torch.allclose(outs[0].cpu().double(), ref, rtol=1e-5, atol=0)
    assert torch.equal(outs[0], outs[1])
    # five times in a tiny captured graph: the same bits (the grid and the order depend on n only)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        hip.prewarm_tickets(torch.device("cuda", 0), ("gradnorm",))
        hip.grad_sumsq(g, 2.0, torch.empty(4, device="cuda"))
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    cap = torch.full((5, 4), -1.0, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        for k in range(5):
            hip.grad_sumsq(g, 2.0, cap[k])
    graph.replay()
    torch.cuda.synchronize()
    for k in range(5):
        assert torch.equal(cap[k], outs[0]), k
    graph.replay()  # and a second replay
    torch.cuda.synchronize()
    assert all(torch.equal(cap[k], outs[0]) for k in range(5))


def test_grad_sumsq_coefficient_edges():
    from dcnn_amd.ops import hip
    out = torch.empty(4, device="cuda")
    hip.grad_sumsq(torch.zeros(4099, device="cuda"), 1.5, out)
    assert out.tolist() == [0.0, 0.0, 1.0, 1.5]  # all-zero gradient: coef 1, no NaN
    g = _randn(4099, 1)
    hip.grad_sumsq(g, 1e30, out)
    assert out[2].item() == 1.0
    g[7] = float("inf")
    hip.grad_sumsq(g, 1.0, out)
    assert out[1].item() == float("inf") and out[2].item() == 0.0  # as torch: max / inf
    g[7] = float("nan")
    hip.grad_sumsq(g, 1.0, out)
    assert out[1].isnan().item() and out[2].isnan().item()  # a NaN norm propagates


def _adam_ref(p, g, m, v, t, wd, decoupled, coef, b1=B1, b2=B2):
    g = g * coef
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    upd = LR * (m / (1 - B1 ** t)) / ((v / (1 - B2 ** t)).sqrt() + EPS)
    if decoupled:
        p = p - wd * LR * p
    else:
        upd = upd + wd * LR * p
    return p - upd, m, v


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("sw", list(SWITCHES))
def test_adam_tail_kernel(n, sw):
    from dcnn_amd.ops import hip
    clip, ema_on = SWITCHES[sw][0] > 0, SWITCHES[sw][1] > 0
    p, g, m, e = _randn(n, 1), _randn(n, 2, 10.0), _randn(n, 3, 0.1), _randn(n, 5)
    v = _randn(n, 4, 0.1).abs()
    nodecay = (torch.rand((n + 63) // 64, generator=torch.Generator().manual_seed(6)) < 0.5).to(torch.uint8).cuda()
    blk = torch.tensor([0.0, 0.0, 0.3, 0.0], device="cuda")
    shadow = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    for decoupled in (True, False):
        pp, mm, vv, ee = p.clone(), m.clone(), v.clone(), e.clone()
        t = 3
        hip.adam_step_tail(pp, g, mm, vv, shadow, LR, B1, B2, EPS, 1 - B1 ** t, 1 - B2 ** t, WD, decoupled, None,
                           nodecay=nodecay, coef=blk[2:3] if clip else None, ema=ee if ema_on else None,
                           ema_decay=DECAY)
        torch.cuda.synchronize()
        wd = torch.where(nodecay.repeat_interleave(64)[:n].bool(), 0.0, WD).double()
        rp, rm, rv = _adam_ref(p.double(), g.double(), m.double(), v.double(), t, wd, decoupled, 0.3 if clip else 1.0)
        assert torch.allclose(pp, rp.float(), **TOL)
        # the moments: the kernel's beta arguments are float32, and 1 - float32(0.999) is 1.3e-5 off
        # 0.001, so their reference takes the float32 values of the betas
        f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))  # noqa: E731
        _, rm, rv = _adam_ref(p.double(), g.double(), m.double(), v.double(), t, wd, decoupled,
                              0.3 if clip else 1.0, f32(B1), f32(B2))
        assert torch.allclose(mm, rm.float(), **TOL) and torch.allclose(vv, rv.float(), **TOL)
        assert torch.equal(shadow, pp.bfloat16())
        if ema_on:
            assert torch.allclose(ee, (DECAY * e.double() + (1 - DECAY) * rp).float(), **TOL)
        else:
            assert torch.equal(ee, e)
        if clip:  # and not the unclipped step
            up, _, _ = _adam_ref(p.double(), g.double(), m.double(), v.double(), t, wd, decoupled, 1.0)
            assert not torch.allclose(pp, up.float(), **TOL)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("sw", list(SWITCHES))
def test_sgd_tail_kernel(n, sw):
    from dcnn_amd.ops import hip
    clip, ema_on = SWITCHES[sw][0] > 0, SWITCHES[sw][1] > 0
    p, g, vel, e = _randn(n, 1), _randn(n, 2, 10.0), _randn(n, 3, 0.1), _randn(n, 5)
    blk = torch.tensor([0.0, 0.0, 0.3, 0.0], device="cuda")
    shadow = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    c = 0.3 if clip else 1.0
    for mom in (MOM, 0.0):
        pp, vv, ee = p.clone(), vel.clone(), e.clone()
        hip.sgd_step_tail(pp, g, vv if mom > 0 else None, shadow, LR, mom, None, coef=blk[2:3] if clip else None,
                          ema=ee if ema_on else None, ema_decay=DECAY)
        torch.cuda.synchronize()
        if mom > 0:
            rv = mom * vel.double() - LR * g.double() * c
            rp = p.double() + rv
            assert torch.allclose(vv, rv.float(), **TOL)
        else:
            rp = p.double() - LR * g.double() * c
            assert torch.equal(vv, vel)
        assert torch.allclose(pp, rp.float(), **TOL) and torch.equal(shadow, pp.bfloat16())
        if ema_on:
            assert torch.allclose(ee, (DECAY * e.double() + (1 - DECAY) * rp).float(), **TOL)
        if clip:
            assert not torch.allclose(pp, (p.double() + (mom * vel.double() if mom > 0 else 0) - LR * g.double()).float(),
                                      **TOL)
    # without clip and EMA the tail kernel computes sgd_kernel's bits
    a, b, va, vb = p.clone(), p.clone(), vel.clone(), vel.clone()
    hip.sgd_step_tail(a, g, va, None, LR, MOM, None)
    hip.sgd_step(b, g, vb, None, LR, MOM)
    assert torch.equal(a, b) and torch.equal(va, vb)


@pytest.mark.parametrize("n", SIZES)
def test_ema_swap_twice_restores_every_bit(n):
    from dcnn_amd.ops import hip
    a, b = _randn(n, 1), _randn(n, 2)
    a[0], b[-1] = float("nan"), -0.0
    a0, b0 = a.clone(), b.clone()
    bits = lambda t: t.view(torch.int32)  # noqa: E731
    shadow = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    hip.ema_swap(a, b, shadow)
    assert torch.equal(bits(a), bits(b0)) and torch.equal(bits(b), bits(a0))
    assert torch.equal(bits(shadow.float()), bits(b0.bfloat16().float()))
    hip.ema_swap(a, b, shadow)
    assert torch.equal(bits(a), bits(a0)) and torch.equal(bits(b), bits(b0))
    assert torch.equal(bits(shadow.float()), bits(a0.bfloat16().float()))
    hip.ema_swap(a, b)  # the shadow is optional
    assert torch.equal(bits(a), bits(b0))


# ------------------------------------------------------------------------------------ model level
@pytest.mark.parametrize("sw", list(SWITCHES))
@pytest.mark.parametrize("kind", KINDS)
def test_three_steps_match_the_formula_gpu(kind, sw):
    m, opt = model_case(kind, sw, "GPU:0")
    assert opt.fused()
    if sw != "ema":
        assert opt.grad_norm_device.is_cuda and opt.grad_norm_device.dtype == torch.float32


@pytest.mark.parametrize("kind", ["adamw_nodecay", "sgd_momentum"])
def test_raw_arena_gpu(kind):
    raw_case(kind, "both", "cuda:0")


@pytest.mark.parametrize("kind", KINDS)
def test_huge_max_norm_is_bit_identical_to_the_plain_step_gpu(kind):
    def run(max_norm):
        m = _model("GPU:0")
        opt = make_opt(kind, max_norm, 0.0)
        opt.attach(m)
        for s in (1, 2, 3):
            set_grads(m.gradients(), s)
            opt.update()
        torch.cuda.synchronize()
        return m, opt
    a, oa = run(1e30)
    b, _ = run(0.0)
    assert oa.grad_norm_device[2].item() == 1.0
    assert torch.equal(a.arena.data, b.arena.data)


def test_switches_off_take_the_old_launch_path_gpu(monkeypatch):
    from dcnn_amd.ops import hip

    def boom(*a, **k):
        raise AssertionError("the tail entry point was reached with both switches off")
    for name in ("adam_step_tail", "sgd_step_tail", "grad_sumsq", "ema_swap"):
        monkeypatch.setattr(hip, name, boom)
    for kind in ("adamw_nodecay", "sgd_momentum"):
        m = _model("GPU:0")
        opt = make_opt(kind, 0.0, 0.0)
        opt.attach(m)
        set_grads(m.gradients(), 1)
        opt.update()
        with opt.ema_weights():
            pass
    torch.cuda.synchronize()


def _net(max_norm, decay):
    from dcnn_amd.nn import AdamW
    m, _, lf = _train_net()
    opt = AdamW(1e-3, weight_decay=WD, no_decay_norm_bias=True, max_grad_norm=max_norm, ema_decay=decay)
    opt.attach(m)
    return m, opt, lf


def test_captured_step_matches_eager():
    """Three replays with clip and EMA on leave the bits of three eager steps in the weights, the EMA
    and the norm block; the warm-up steps of the capture did not average; both off is another run."""
    from dcnn_amd.runtime.step import TrainStep
    torch.manual_seed(3)
    xs = [torch.randn(8, 3, 16, 16, device="cuda") for _ in range(3)]
    ys = [torch.randint(0, 10, (8,), device="cuda") for _ in range(3)]
    m, opt, lf = _net(0.05, DECAY)
    st = TrainStep(m, lf, opt, use_graph=False)
    m2, opt2, lf2 = _net(0.05, DECAY)
    st2 = TrainStep(m2, lf2, opt2, use_graph=True)
    init = m2.arena.data.clone()
    st2._capture(xs[0], ys[0])
    torch.cuda.synchronize()
    # before the first replay: warm-up rolled the weights AND the EMA back
    assert st2.graphs is not None and torch.equal(m2.arena.data, init) and torch.equal(opt2.ema[0], init)
    coefs = []
    for x, y in zip(xs, ys):
        st(x, y)
        st2(x, y)
        torch.cuda.synchronize()
        assert torch.equal(opt.grad_norm_device, opt2.grad_norm_device)
        coefs.append(opt.grad_norm_device[2].item())
    assert opt.t == opt2.t == 3 and min(coefs) < 1.0  # the clip was active
    assert torch.equal(m.arena.data, m2.arena.data) and torch.equal(opt.ema[0], opt2.ema[0])
    assert not torch.equal(opt.ema[0], m.arena.data) and not torch.equal(opt.ema[0], init)
    m3, opt3, lf3 = _net(0.0, 0.0)
    st3 = TrainStep(m3, lf3, opt3, use_graph=False)
    for x, y in zip(xs, ys):
        st3(x, y)
    torch.cuda.synchronize()
    assert not torch.equal(m.arena.data, m3.arena.data)

    # validation inside ema_weights() == the forward of a second model whose arena was filled from the EMA
    x = xs[0]
    m.set_training(False)
    with torch.no_grad():
        live = m.forward(x).float().clone()
        data, ema, shadow = m.arena.data.clone(), opt.ema[0].clone(), m.arena.shadow.clone()
        with opt.ema_weights():
            assert torch.equal(m.arena.data, ema)
            avg = m.forward(x).float().clone()
        torch.cuda.synchronize()
        # after: every bit of data, ema and the shadow is restored
        assert torch.equal(m.arena.data, data) and torch.equal(opt.ema[0], ema) and torch.equal(m.arena.shadow, shadow)
        m4, _, _ = _net(0.0, 0.0)
        m4.arena.data.copy_(ema)
        m4.arena.sync_shadow(force=True)
        m4.set_training(False)
        want = m4.forward(x).float()
    assert torch.equal(avg, want) and not torch.equal(avg, live)
