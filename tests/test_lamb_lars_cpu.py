"""LAMB and LARS on the CPU: the native flat-buffer steps of an arena (ops/cpu.py lamb_step / lars_step,
driven by the shared segment / chunk tables) and the per-parameter fallback of nn/optimizers.py, against
a float64 per-parameter formula written here (never the code under test):

  LAMB  m = b1 m + (1 - b1) g,  v = b2 v + (1 - b2) g g,  r = (m / bc1) / (sqrt(v / bc2) + eps) + wd_i p
        trust_i = ||p_i|| / ||r_i|| if adapt_i and ||p_i|| != 0 and ||r_i|| != 0 else 1,  p -= lr trust_i r
  LARS  trust_i = tc ||p_i|| / (||g_i|| + wd_i ||p_i|| + eps) if adapt_i and ||p_i|| != 0 and ||g_i|| != 0 else 1
        v = mom v - lr trust_i (g + wd_i p),  p += v

with wd_i = 0 and adapt_i = false for a flagged parameter when ``no_decay_norm_bias`` is on. A NaN norm
is not zero: it propagates into that parameter's step. The gradients of the three steps are randn times
1, 100 and 0.01 (the helpers of test_clip_ema_cpu.py); every "matches the formula" test also asserts
that the result does NOT match plain Adam / SGD with L2, so the trust ratio demonstrably acted."""
import math
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_clip_ema_cpu import TOL, _dp_batch, _dp_model, _free_port, set_grads
from test_decay_exclusion import EXPECTED, _model, _raw_arena

LR, B1, B2, EPS, WD = 0.01, 0.9, 0.999, 1e-6, 0.1
LARS_LR, MOM, TC, LARS_EPS = 0.5, 0.9, 0.02, 1e-8
SEVEN = (1, 63, 64, 65, 4096, 4097, 3 * 4096 + 5)
KINDS = ["lamb", "lamb_nodecay", "lars", "lars_nodecay", "lars_nomomentum"]


def make_opt(kind, max_norm=0.0, decay=0.0):
    from dcnn_amd.nn import LAMB, LARS
    nd = kind.endswith("_nodecay")
    if kind.startswith("lamb"):
        return LAMB(LR, B1, B2, EPS, WD, no_decay_norm_bias=nd, max_grad_norm=max_norm, ema_decay=decay)
    return LARS(LARS_LR, 0.0 if kind == "lars_nomomentum" else MOM, WD, TC, LARS_EPS, no_decay_norm_bias=nd,
                max_grad_norm=max_norm, ema_decay=decay)


def _l2(t):
    return math.sqrt(float((t * t).sum()))


def reference(kind, p0, grads_per_step, no_decay, trust_on=True, hyper=None, state=None, coefs=None):
    """float64, per parameter. Returns (params, state dict, [trust ratios per step]). ``trust_on=False``
    is plain Adam with L2 in LAMB's form / SGD with L2: what the step would be without the ratio.
    ``hyper``: overrides of the module constants; ``state``: (t0, m, v) to continue from; ``coefs``: a clip
    coefficient per step."""
    h = dict(lr=LR, b1=B1, b2=B2, eps=EPS, wd=WD, lars_lr=LARS_LR, mom=MOM, tc=TC, lars_eps=LARS_EPS)
    h.update(hyper or {})
    lamb = kind.startswith("lamb")
    nd = kind.endswith("_nodecay")
    mom = 0.0 if kind == "lars_nomomentum" else h["mom"]
    ref = [p.clone().double() for p in p0]
    t0 = 0
    mm = [torch.zeros_like(r) for r in ref]
    vv = [torch.zeros_like(r) for r in ref]
    if state is not None:
        t0, mm, vv = state[0], [x.clone().double() for x in state[1]], [x.clone().double() for x in state[2]]
    trusts = []
    for s, grads in enumerate(grads_per_step):
        t = t0 + s + 1
        c = 1.0 if coefs is None else coefs[s]
        bc1, bc2 = 1 - h["b1"] ** t, 1 - h["b2"] ** t
        row = []
        for i, g in enumerate(grads):
            g = g.double() * c
            flagged = nd and no_decay[i]
            wd, adapt = (0.0, False) if flagged else (h["wd"], True)
            pn = _l2(ref[i])
            trust = 1.0
            if lamb:
                mm[i] = h["b1"] * mm[i] + (1 - h["b1"]) * g
                vv[i] = h["b2"] * vv[i] + (1 - h["b2"]) * g * g
                r = (mm[i] / bc1) / ((vv[i] / bc2).sqrt() + h["eps"]) + wd * ref[i]
                rn = _l2(r)
                if adapt and trust_on and not (pn == 0.0 or rn == 0.0):
                    trust = pn / rn
                ref[i] = ref[i] - h["lr"] * trust * r
            else:
                gn = _l2(g)
                if adapt and trust_on and not (pn == 0.0 or gn == 0.0):
                    trust = h["tc"] * pn / (gn + wd * pn + h["lars_eps"])
                u = g + wd * ref[i]
                if mom > 0:
                    mm[i] = mom * mm[i] - h["lars_lr"] * trust * u
                    ref[i] = ref[i] + mm[i]
                else:
                    ref[i] = ref[i] - h["lars_lr"] * trust * u
            row.append(trust)
        trusts.append(row)
    return ref, dict(t=t0 + len(grads_per_step), m=mm, v=vv), trusts


def state_views(kind, opt, view):
    """the optimizer's state tensors per parameter, as the formula names them"""
    n = len(opt.params)
    if kind.startswith("lamb"):
        if opt.arena is not None:
            return {"m": [view(opt.m[0], i) for i in range(n)], "v": [view(opt.v[0], i) for i in range(n)]}
        return {"m": opt.m, "v": opt.v}
    if opt.velocity is None:
        return {}
    return {"m": [view(opt.velocity[0], i) for i in range(n)] if opt.arena is not None else opt.velocity}


def check_run(kind, params, grad_tensors, opt, p0, no_decay, view, sync=lambda: None):
    """Three steps; parameters, state and last_trust_ratios() after EACH step against the formula."""
    per_step = []
    for s in (1, 2, 3):
        per_step.append(set_grads(grad_tensors, s))
        before = [g.detach().cpu().clone() for g in grad_tensors]
        opt.update()
        sync()
        assert all(torch.equal(a, g.detach().cpu()) for a, g in zip(before, grad_tensors))  # g is not rewritten
        ref, st, trusts = reference(kind, p0, per_step, no_decay)
        for i, (p, r) in enumerate(zip(params, ref)):
            assert torch.allclose(p.detach().cpu().double(), r, **TOL), (s, i, "params")
        for key, ts in state_views(kind, opt, view).items():
            for i, (a, r) in enumerate(zip(ts, st[key])):
                assert torch.allclose(a.detach().cpu().double(), r, **TOL), (s, i, key)
        got = opt.last_trust_ratios()
        assert len(got) == len(params)
        assert got == pytest.approx(trusts[-1], rel=1e-5), (s, "trust")
    if kind.endswith("_nodecay"):
        assert all(t == 1.0 for t, f in zip(got, no_decay) if f)
    assert any(abs(t - 1.0) > 0.05 for t in got)
    plain, _, _ = reference(kind, p0, per_step, no_decay, trust_on=False)
    assert not all(torch.allclose(p.detach().cpu().double(), r, **TOL) for p, r in zip(params, plain))
    return per_step


def model_case(kind, device=None):
    m = _model(device)
    sync = torch.cuda.synchronize if device is not None else (lambda: None)
    p0 = [p.detach().cpu().clone() for p in m.parameters()]
    opt = make_opt(kind)
    opt.attach(m)
    assert opt.arena is m.arena
    check_run(kind, m.parameters(), m.gradients(), opt, p0, EXPECTED, m.arena._view, sync)
    return m, opt


def raw_case(kind, device="cpu"):
    ar = _raw_arena(device)
    sync = torch.cuda.synchronize if str(device) != "cpu" else (lambda: None)
    p0 = [ar.param(i).detach().cpu().clone() for i in range(3)]
    opt = make_opt(kind)
    params, grads = [ar.param(i) for i in range(3)], [ar.grad_view(i) for i in range(3)]
    opt.attach(params, grads, ar)
    assert opt.arena is ar
    check_run(kind, params, grads, opt, p0, [False, True, False], ar._view, sync)
    flat = ar.data.cpu()  # the padding between the slices stays zero
    assert (flat[70:128] == 0).all() and (flat[200:] == 0).all()


@pytest.mark.parametrize("kind", KINDS)
def test_three_steps_match_the_formula_model(kind):
    model_case(kind)


@pytest.mark.parametrize("kind", KINDS)
def test_three_steps_match_the_formula_raw_arena(kind):
    raw_case(kind)


@pytest.mark.parametrize("kind", KINDS)
def test_per_parameter_fallback(kind):
    m = _model()
    p0 = [p.detach().clone() for p in m.parameters()]
    params = [p.clone() for p in p0]
    grads = [torch.zeros_like(p) for p in p0]
    opt = make_opt(kind)
    opt.attach(params, grads, no_decay=EXPECTED)
    assert opt.arena is None
    check_run(kind, params, grads, opt, p0, EXPECTED, None)


@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_float64_arena(kind):
    from dcnn_amd.nn.params import ParamArena, ParamSpec
    specs = [ParamSpec("a", (70,)), ParamSpec("b", (5000,), no_decay=True)]
    ar = ParamArena(specs, torch.device("cpu"), dtype=torch.float64)
    g = torch.Generator().manual_seed(4)
    for i in range(2):
        ar.param(i).copy_(torch.randn(specs[i].shape, generator=g))
    p0 = [ar.param(i).detach().clone() for i in range(2)]
    opt = make_opt(kind + "_nodecay")
    params, grads = [ar.param(i) for i in range(2)], [ar.grad_view(i) for i in range(2)]
    opt.attach(params, grads, ar)
    per_step = [set_grads(grads, s) for s in (1,)]
    opt.update()
    ref, _, trusts = reference(kind + "_nodecay", p0, per_step, [False, True])
    for p, r in zip(params, ref):
        assert torch.allclose(p, r, atol=1e-12, rtol=1e-11)
    assert opt.last_trust_ratios() == pytest.approx(trusts[0], rel=1e-12)


# ------------------------------------------------------------------------------------ edge cases
def _edge_arena(device="cpu"):
    from dcnn_amd.nn.params import ParamArena, ParamSpec
    specs = [ParamSpec("zero", (70,)), ParamSpec("w", (130,)), ParamSpec("flagged", (64,), no_decay=True),
             ParamSpec("w2", (5000,))]
    ar = ParamArena(specs, torch.device(device))
    g = torch.Generator().manual_seed(21)
    for i in (1, 2, 3):
        ar.param(i).copy_(torch.randn(specs[i].shape, generator=g))
    return ar, [ar.param(i) for i in range(4)], [ar.grad_view(i) for i in range(4)]


def edge_cases(kind, device="cpu", arena=True):
    sync = torch.cuda.synchronize if str(device) != "cpu" else (lambda: None)

    def fresh(wd):
        ar, params, grads = _edge_arena(device)
        from dcnn_amd.nn import LAMB, LARS
        opt = (LAMB(LR, B1, B2, EPS, wd, no_decay_norm_bias=True) if kind == "lamb"
               else LARS(LARS_LR, MOM, wd, TC, LARS_EPS, no_decay_norm_bias=True))
        if arena:
            opt.attach(params, grads, ar)
        else:
            params = [p.detach().clone() for p in params]
            grads = [torch.zeros_like(p) for p in params]
            opt.attach(params, grads, no_decay=[False, False, True, False])
        return opt, params, grads
    nd = [False, False, True, False]
    # an all-zero parameter: trust 1 (it still takes the step); a flagged one: trust 1 and no decay
    opt, params, grads = fresh(WD)
    p0 = [p.detach().cpu().clone() for p in params]
    per = [set_grads(grads, 1)]
    opt.update()
    sync()
    ref, _, trusts = reference(kind + "_nodecay", p0, per, nd)
    tr = opt.last_trust_ratios()
    assert tr[0] == 1.0 and tr[2] == 1.0 and trusts[0][0] == 1.0 and trusts[0][2] == 1.0
    assert tr[1] != 1.0 and tr[3] != 1.0 and tr == pytest.approx(trusts[0], rel=1e-5)
    for p, r in zip(params, ref):
        assert torch.allclose(p.detach().cpu().double(), r, **TOL)
    decayed, _, _ = reference(kind, p0, per, nd)  # the flagged parameter decayed and adapted: another result
    assert not torch.allclose(params[2].detach().cpu().double(), decayed[2], **TOL)
    # a zero gradient with wd = 0: trust 1 and nothing moves
    opt, params, grads = fresh(0.0)
    p0 = [p.detach().cpu().clone() for p in params]
    for g in grads:
        g.zero_()
    opt.update()
    sync()
    assert opt.last_trust_ratios() == [1.0, 1.0, 1.0, 1.0]
    assert all(torch.equal(p.detach().cpu(), q) for p, q in zip(params, p0))
    # a NaN in one parameter's gradient poisons that parameter only (the norm propagates: every element)
    opt, params, grads = fresh(WD)
    set_grads(grads, 1)
    grads[3].view(-1)[4321 if arena else 17] = float("nan")
    opt.update()
    sync()
    tr = opt.last_trust_ratios()
    assert math.isnan(tr[3]) and all(math.isfinite(t) for t in tr[:3])
    assert torch.isnan(params[3].detach().cpu()).all()
    assert all(torch.isfinite(p.detach().cpu()).all() for p in params[:3])


@pytest.mark.parametrize("arena", [True, False], ids=["arena", "per_parameter"])
@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_edge_cases(kind, arena):
    edge_cases(kind, arena=arena)


# ------------------------------------------------------------------------------------ the tables
def seven_slice_tables(device="cpu", exclude=False, flags=None):
    from dcnn_amd.nn.params import SegmentTables
    offs, off = [], 0
    for n in SEVEN:
        offs.append(off)
        off += (n + 63) // 64 * 64
    return SegmentTables.from_slices(offs, list(SEVEN), flags, exclude, off, device), offs, off


def check_tables(t, offs, counts, total):
    """the chunks tile the slices exactly, none straddles a slice, each segment's rows are contiguous"""
    chunks, segs = t.chunks.tolist(), t.segs.tolist()
    assert t.cover == total and len(segs) == len(counts)
    covered = torch.zeros(total // 64, dtype=torch.int32)
    for c, (first, blocks, seg) in enumerate(chunks):
        assert 1 <= blocks <= 64
        lo, hi = offs[seg] // 64, (offs[seg] + counts[seg] + 63) // 64
        assert lo <= first and first + blocks <= hi, (c, "straddles a slice")
        covered[first:first + blocks] += 1
        assert segs[seg][0] <= c < segs[seg][0] + segs[seg][1]
    assert (covered == 1).all()
    nxt = 0
    for s, (first, n, _, _) in enumerate(segs):
        assert first == nxt and n == (counts[s] + 4095) // 4096
        assert [c[2] for c in chunks[first:first + n]] == [s] * n  # contiguous, in arena order
        assert [c[0] for c in chunks[first:first + n]] == [offs[s] // 64 + 64 * k for k in range(n)]
        nxt += n
    assert nxt == len(chunks)


def test_segment_table_seven_slices():
    t, offs, total = seven_slice_tables()
    check_tables(t, offs, SEVEN, total)
    assert t.nchunks == 1 + 1 + 1 + 1 + 1 + 2 + 4
    assert all(s[2] == 1 and s[3] == 1 for s in t.segs.tolist())
    flags = [0, 1, 0, 0, 1, 0, 0]
    on, _, _ = seven_slice_tables(exclude=True, flags=flags)
    assert [s[2] for s in on.segs.tolist()] == [1 - f for f in flags] == [s[3] for s in on.segs.tolist()]
    off, _, _ = seven_slice_tables(exclude=False, flags=flags)
    assert torch.equal(off.segs, t.segs) and torch.equal(on.chunks, t.chunks)


def test_segment_table_of_an_arena_is_cached_and_checked():
    from dcnn_amd.nn.params import SegmentTables
    from dcnn_amd.ops._ext import kernels
    m = _model()
    t = m.arena.segment_tables(True)
    assert m.arena.segment_tables(True) is t and m.arena.segment_tables(False) is not t
    counts = [p.numel() for p in m.parameters()]
    check_tables(t, m.arena.offsets, counts, m.arena.numel)
    assert [bool(1 - s[2]) for s in t.segs.tolist()] == EXPECTED
    with pytest.raises(ValueError, match="aligned"):
        SegmentTables.from_slices([0, 70], [70, 8], None, False, 256, "cpu")
    with pytest.raises(ValueError, match="ends at element 192 of an arena of 128"):
        SegmentTables.from_slices([0, 128], [70, 8], None, False, 128, "cpu")
    kernels().optim_segments_check(t.chunks.flatten().tolist(), t.segs.flatten().tolist(), m.arena.numel)
    with pytest.raises(ValueError, match="does not fit"):
        kernels().optim_segments_check(t.chunks.flatten().tolist(), t.segs.flatten().tolist(), m.arena.numel - 64)
    from dcnn_amd.ops import cpu
    with pytest.raises(ValueError, match="reaches element"):
        n = m.arena.numel - 64
        z = torch.zeros(n)
        cpu.lars_step(z, z.clone(), None, 0.1, 0.0, 0.0, 1e-3, 1e-8, t, torch.ones(3 * t.nsegs, dtype=torch.float64))


# ------------------------------------------------------------------------ interfaces and state
def test_config_factory_clone():
    from dcnn_amd.nn import LAMB, LARS, OptimizerFactory
    a, b = LAMB(), LARS()
    assert (a.learning_rate, a.beta1, a.beta2, a.epsilon, a.weight_decay) == (1e-3, 0.9, 0.999, 1e-6, 0.01)
    assert (b.learning_rate, b.momentum, b.weight_decay, b.trust_coefficient, b.epsilon) == (0.1, 0.9, 5e-4, 1e-3, 1e-8)
    for o in (a, b):
        assert not o.no_decay_norm_bias and o.max_grad_norm == 0.0 and o.ema_decay == 0.0
    assert a.get_config()["type"] == "lamb" and b.get_config()["type"] == "lars"
    for o in (LAMB(0.002, 0.8, 0.99, 1e-5, 0.05, True, 2.5, 0.99), LARS(0.3, 0.8, 1e-4, 0.002, 1e-7, True, 2.5, 0.99)):
        cfg = o.get_config()
        for o2 in (OptimizerFactory.create_from_config(cfg.to_json()), o.clone()):
            assert type(o2) is type(o) and dict(o2.get_config()) == dict(cfg)
    assert isinstance(OptimizerFactory.create_from_config({"type": "lamb", "parameters": {}}), LAMB)
    assert isinstance(OptimizerFactory.create_from_config({"type": "lars", "parameters": {}}), LARS)
    with pytest.raises(ValueError, match="no_decay_norm_bias"):
        LAMB(no_decay_norm_bias=True).attach([torch.zeros(3)], [torch.zeros(3)])


@pytest.mark.parametrize("kind", ["lamb_nodecay", "lars"])
def test_state_save_and_resume_bit_for_bit(kind, tmp_path):
    """two steps, a .state checkpoint, one more step == three steps, bit for bit"""
    from dcnn_amd.nn.train import load_checkpoint, save_checkpoint

    def steps(m, opt, which):
        for s in which:
            set_grads(m.gradients(), s)
            opt.update()
    m = _model()
    opt = make_opt(kind)
    opt.attach(m)
    steps(m, opt, (1, 2))
    path = str(tmp_path / "ckpt")
    save_checkpoint(m, opt, path, epoch=1)
    steps(m, opt, (3,))
    m2 = _model()
    opt2 = make_opt(kind)
    assert load_checkpoint(m2, opt2, path) == 1
    assert sorted(opt2.state_dict()) == (["m", "t", "v"] if kind.startswith("lamb") else ["velocity"])
    steps(m2, opt2, (3,))
    assert torch.equal(m.arena.data, m2.arena.data)
    if kind.startswith("lamb"):
        assert opt2.t == 3 and torch.equal(opt.m[0], opt2.m[0]) and torch.equal(opt.v[0], opt2.v[0])
    else:
        assert torch.equal(opt.velocity[0], opt2.velocity[0])
    assert opt.last_trust_ratios() == opt2.last_trust_ratios()


@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_flat_optimizer_state_round_trip(kind):
    """the pipeline stages' flat state transfer carries LAMB's / LARS's state by key"""
    from dcnn_amd.parallel.pipeline.stage import flat_optimizer_state, load_flat_optimizer_state
    m, opt = model_case(kind)
    flat = flat_optimizer_state(opt)
    n = m.arena.numel
    assert flat.numel() == 2 + (2 * n if kind == "lamb" else n)
    m2 = _model()
    opt2 = make_opt(kind)
    opt2.attach(m2)
    load_flat_optimizer_state(opt2, flat)
    a, b = opt.state_dict(), opt2.state_dict()
    assert sorted(a) == sorted(b)
    for k in a:
        if isinstance(a[k], list):
            assert all(torch.equal(x, y) for x, y in zip(a[k], b[k]))
        else:
            assert a[k] == b[k]


def test_clip_and_ema_ride_along():
    """max_grad_norm: the coefficient multiplies g at the load (LARS: coef ||g||); ema: updated in the
    applying pass. Against the formula with the coefficient of each step."""
    from test_clip_ema_cpu import DECAY, MAXN
    for kind in ("lamb", "lars"):
        m = _model()
        p0 = [p.detach().clone() for p in m.parameters()]
        opt = make_opt(kind, MAXN, DECAY)
        opt.attach(m)
        per, coefs = [], []
        ema = [p.clone().double() for p in p0]
        for s in (1, 2, 3):
            per.append(set_grads(m.gradients(), s))
            norm = math.sqrt(sum(float((g.double() ** 2).sum()) for g in per[-1]))
            coefs.append(min(1.0, MAXN / (norm + 1e-6)))
            opt.update()
            ref, _, trusts = reference(kind, p0, per, EXPECTED, coefs=coefs)
            ema = [DECAY * e + (1 - DECAY) * r for e, r in zip(ema, ref)]
            assert opt.last_trust_ratios() == pytest.approx(trusts[-1], rel=1e-5)
        assert coefs[0] < 1 and coefs[1] < 0.01 and coefs[2] == 1.0
        for i, (p, r) in enumerate(zip(m.parameters(), ref)):
            assert torch.allclose(p.double(), r, **TOL), (kind, i)
        for i, e in enumerate(ema):
            assert torch.allclose(m.arena._view(opt.ema[0], i).double(), e, **TOL), (kind, i, "ema")


def test_rollback_list_covers_the_state():
    """runtime/step.py rolls the warm-up steps back by attribute name: m, v, velocity, ema"""
    m = _model()
    for kind, names in (("lamb", ("m", "v")), ("lars", ("velocity",))):
        opt = make_opt(kind, 0.0, 0.5)
        opt.attach(m)
        held = {id(t) for name in ("m", "v", "velocity", "ema") for t in (getattr(opt, name, None) or [])}
        for name in names + ("ema",):
            assert all(id(t) in held for t in getattr(opt, name))
        assert set(k for k, v in opt.state_dict().items() if isinstance(v, list)) == set(names) | {"ema"}
        assert opt.layerwise is True


# ------------------------------------------------------------------------------- data parallel
def _dp_opt(kind):
    from dcnn_amd.nn import LAMB, LARS
    return LAMB(0.01, weight_decay=0.1) if kind == "lamb" else LARS(0.5, 0.9, 0.1, 0.02)


def _dp_worker(rank, world, port, out_dir, kind):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from dcnn_amd.nn import LossFactory
    from dcnn_amd.parallel.dp import DataParallel
    from dcnn_amd.runtime.step import TrainStep
    model = _dp_model(100 + rank)  # different init per rank: the broadcast unifies it
    dp = DataParallel(model, bucket_mb=0.001)
    opt = _dp_opt(kind)
    opt.attach(model)
    step = TrainStep(dp, LossFactory.create("softmax_crossentropy"), opt)
    x, y = _dp_batch()
    step(x[rank * 4:(rank + 1) * 4], y[rank * 4:(rank + 1) * 4])
    torch.save({"params": [p.detach().clone() for p in model.parameters()], "trust": opt.last_trust_ratios(),
                "nbuckets": len(dp.buckets)}, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_dp_two_ranks_equal_the_whole_batch_step(kind, tmp_path):
    """World size 2 over gloo: the norms are taken behind the all-reduce, on the averaged gradient, so
    the step on two half-batches equals the single-process step on the whole batch."""
    mp.spawn(_dp_worker, args=(2, _free_port(), str(tmp_path), kind), nprocs=2, join=True)
    r0 = torch.load(tmp_path / "rank0.pt", weights_only=True)
    r1 = torch.load(tmp_path / "rank1.pt", weights_only=True)
    assert r0["nbuckets"] > 1 and r0["trust"] == r1["trust"]
    for a, b in zip(r0["params"], r1["params"]):
        assert torch.equal(a, b)
    from dcnn_amd.nn import LossFactory
    ref = _dp_model(100)
    opt = _dp_opt(kind)
    opt.attach(ref)
    x, y = _dp_batch()
    opt.clear_gradients()
    _, grad, _ = LossFactory.create("softmax_crossentropy").loss_and_grad(ref.forward(x), y)
    ref.backward(grad)
    opt.update()
    assert r0["trust"] == pytest.approx(opt.last_trust_ratios(), rel=1e-5)
    assert any(abs(t - 1.0) > 0.05 for t in r0["trust"])
    for a, b in zip(r0["params"], ref.parameters()):
        assert torch.allclose(a, b, **TOL)


# ------------------------------------------------------------------------------------ pipeline
def test_two_stage_pipeline_with_lamb_matches_single_process():
    """A trust ratio is local to a parameter, so a stage's step is the model's step: a two-stage
    in-process pipeline with "lamb" equals the single-process run (tests/test_pipeline.py's parity
    tolerance: losses rel 1e-5, parameters rtol 1e-5 / atol 1e-6)."""
    from dcnn_amd.models import zoo
    from dcnn_amd.nn import LAMB
    from dcnn_amd.parallel.pipeline import InProcessCoordinator
    from test_pipeline import _reference_microbatched
    torch.manual_seed(0)
    model = zoo.create_model("mnist_cnn")
    model.set_seed(3)
    model.initialize()
    ref = model.clone()
    ref.initialize()
    ref.load_parameters([p.clone() for p in model.parameters()])
    x = torch.randn(8, 1, 28, 28)
    y = torch.randint(0, 10, (8,))
    coord = InProcessCoordinator(model, LAMB(1e-3, weight_decay=0.05, no_decay_norm_bias=True),
                                 "softmax_crossentropy", num_stages=2, num_microbatches=4, transport="local")
    try:
        coord.initialize()
        coord.deploy_stages()
        coord.send_parameters(model)
        coord.start()
        losses = [coord.train_step(x, y, "sync") for _ in range(2)]
        ref_opt = LAMB(1e-3, weight_decay=0.05, no_decay_norm_bias=True)
        ref_losses = [_reference_microbatched(ref, x, y, 4, ref_opt) for _ in range(2)]
        assert losses == pytest.approx(ref_losses, rel=1e-5)
        got = coord.gather_model()
        for a, b in zip(got.parameters(), ref.parameters()):
            torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)
        assert any(abs(t - 1.0) > 0.05 for t in ref_opt.last_trust_ratios())
    finally:
        coord.stop()


def test_pipeline_stage_accepts_both_and_still_refuses_the_switches():
    from dcnn_amd.nn import LAMB, LARS
    from dcnn_amd.parallel.pipeline.config import StageConfig
    from dcnn_amd.parallel.pipeline.stage import PipelineStage

    class _Comm:
        id = "stage_0"

        def send(self, m):
            pass

    m = _model()
    for opt in (LAMB(), LARS()):
        st = PipelineStage(_Comm())
        st._configure(StageConfig("stage_0", 0, 1, m.get_config(), dict(opt.get_config())).dumps())
        assert type(st.optimizer) is type(opt)
    for opt, key in ((LAMB(max_grad_norm=1.0), "max_grad_norm"), (LARS(ema_decay=0.5), "ema_decay")):
        st = PipelineStage(_Comm())
        with pytest.raises(ValueError, match=key):
            st._configure(StageConfig("stage_0", 0, 1, m.get_config(), dict(opt.get_config())).dumps())
