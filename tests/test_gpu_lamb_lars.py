"""LAMB and LARS on the GPU: the raw two-launch steps of layerwise.hip over tables made for the
purpose, against float64 formulas; bit-reproducibility eager / captured; every combination of the
optional inputs; the three-step model tests of tests/test_lamb_lars_cpu.py on GPU:0; the captured
TrainStep against eager steps.

Arenas: one segment of 64 elements (one ragged chunk, one workgroup); the seven slices 1, 63, 64, 65,
4096, 4097, 3 * 4096 + 5 (full and ragged chunks, one to four chunks a segment); 1100 segments of 64
elements (more segments than the finishing workgroup has lanes: 1024, or waves: 16; 1100 chunks over a
grid of 512, so workgroups loop); one segment of 2**20 + 64 elements (257 chunks in one segment, the
last of one block).

RTOL of the trust table and the sums against float64, from the kernel's own chains: an element's
square is one rounding; a lane adds its four squares in 2 levels; the wave butterfly has 6 levels and
the sixteen wave sums 4: 13 roundings to a chunk's partial. The finishing wave's lane adds at most
ceil(257 / 64) = 5 partials in sequence, then 6 butterfly levels: 24 roundings on a sum of
non-negative terms, 24 * 2^-24 relative. LARS's sums have exact inputs. LAMB's r carries the fp32
roundings of m, v (3 each), two divisions, a square root and two additions: |dr| <= ~10 * 2^-24 of
the magnitudes that formed it, which by Cauchy-Schwarz is <= ~2 * 10 * 2^-24 relative on sum r^2 for
data without systematic cancellation (the moments and the gradient here are independent draws). So
sums are within (24 + 20) * 2^-24 and a trust ratio (two square roots halve it, two roundings, one
division, tc and eps two more) within about 50 * 2^-24: RTOL = 64 * 2^-24 = 2^-18 ~ 3.8e-6 for both."""
import itertools

import pytest
import torch

from test_clip_ema_cpu import TOL, set_grads
from test_decay_exclusion import _model, _train_net
from test_lamb_lars_cpu import KINDS, SEVEN, edge_cases, make_opt, model_case, raw_case

pytestmark = pytest.mark.gpu
RTOL = 2.0 ** -18
LR, B1, B2, EPS, WD, BC1, BC2 = 0.01, 0.9, 0.999, 1e-6, 0.1, 0.19, 0.002
MOM, TC, LARS_EPS, DECAY = 0.9, 0.02, 1e-8, 0.9
ARENAS = {"one64": (64,), "seven": SEVEN, "many": (64,) * 1100, "long": (2 ** 20 + 64,)}
DEV = "cuda:0"


def f32(x):
    """the float32 a kernel argument is rounded to, as a Python float"""
    return float(torch.tensor(x, dtype=torch.float32))


def layout(name):
    """(offsets, counts, total, flags) of arena ``name``: slices 64-element aligned, every third flagged"""
    counts = ARENAS[name]
    offs, off = [], 0
    for n in counts:
        offs.append(off)
        off += (n + 63) // 64 * 64
    return offs, counts, off, [i % 3 == 1 for i in range(len(counts))] if len(counts) > 1 else [False]


def make_tables(name, exclude=True, device=DEV):
    from dcnn_amd.nn.params import SegmentTables
    offs, counts, total, flags = layout(name)
    return SegmentTables.from_slices(offs, list(counts), flags, exclude, total, device)


_STATE = {}


def state_of(name):
    """p, g, m, v, vel, ema (CPU float32, zero in the gaps between slices), computed once and shared"""
    if name not in _STATE:
        offs, counts, total, _ = layout(name)
        gen = torch.Generator().manual_seed(len(name) + total)
        mask = torch.zeros(total)
        for o, n in zip(offs, counts):
            mask[o:o + n] = 1
        st = {k: torch.randn(total, generator=gen) * sc * mask
              for k, sc in (("p", 0.5), ("g", 2.0), ("m", 0.1), ("vel", 0.05), ("ema", 0.5))}
        st["v"] = (torch.randn(total, generator=gen) * 0.3) ** 2 * mask
        _STATE[name] = st
    return _STATE[name]


def reference(kind, name, coef, ema, mom=MOM):
    """float64 per segment from the float32 inputs. Returns dict p, m, v | vel, ema, trust, sums."""
    offs, counts, total, flags = layout(name)
    st = {k: x.double() for k, x in state_of(name).items()}
    lr, b1, b2, eps, wd, bc1, bc2 = (f32(x) for x in (LR, B1, B2, EPS, WD, BC1, BC2))
    k1, k2 = f32(1 - B1), f32(1 - B2)  # the kernel takes float(1 - beta), rounded from double
    mo, tc, leps, d = f32(mom), f32(TC), f32(LARS_EPS), f32(DECAY)
    c = f32(coef) if coef is not None else 1.0
    out = {k: st[k].clone() for k in ("p", "m", "v", "vel", "ema")}
    trust, sums = [], []
    for o, n, flagged in zip(offs, counts, flags):
        sl = slice(o, o + n)
        p, g = st["p"][sl], st["g"][sl]
        w, adapt = (0.0, False) if flagged else (wd, True)
        sp = float((p * p).sum())
        if kind == "lamb":
            gc = g * c
            m = b1 * st["m"][sl] + k1 * gc
            v = b2 * st["v"][sl] + k2 * gc * gc
            r = (m / bc1) / ((v / bc2).sqrt() + eps) + w * p
            su = float((r * r).sum())
            t = (sp / su) ** 0.5 if adapt and sp != 0 and su != 0 else 1.0
            out["m"][sl], out["v"][sl] = m, v
            out["p"][sl] = p - lr * t * r
        else:
            su = float((g * g).sum())
            pn, gn = sp ** 0.5, c * su ** 0.5
            t = tc * pn / (gn + w * pn + leps) if adapt and pn != 0 and gn != 0 else 1.0
            u = g * c + w * p
            if mo > 0:
                out["vel"][sl] = mo * st["vel"][sl] - lr * t * u
                out["p"][sl] = p + out["vel"][sl]
            else:
                out["p"][sl] = p - lr * t * u
        trust.append(t)
        sums.append((sp, su))
    if ema:
        out["ema"] = d * st["ema"] + (1 - d) * out["p"]
    out["trust"], out["sums"] = trust, sums
    return out


def launch(kind, t, bufs, ws, coef, ema, hyper, mom=MOM):
    """one step on the current stream. With ``hyper`` the scalar arguments it overrides are wrong on
    purpose: the kernels must read the device values."""
    from dcnn_amd.ops import hip
    trust, part = ws
    e = bufs["ema"] if ema else None
    if kind == "lamb":
        lr, bc1, bc2 = (999.0, 0.5, 0.5) if hyper is not None else (LR, BC1, BC2)
        hip.lamb_step(bufs["p"], bufs["g"], bufs["m"], bufs["v"], bufs["shadow"], lr, B1, B2, EPS, bc1, bc2, WD, t,
                      trust, part, hyper=hyper, coef=coef, ema=e, ema_decay=DECAY if ema else 0.0)
    else:
        hip.lars_step(bufs["p"], bufs["g"], bufs["vel"] if mom > 0 else None, bufs["shadow"],
                      999.0 if hyper is not None else LR, mom, WD, TC, LARS_EPS, t, trust, part, hyper=hyper,
                      coef=coef, ema=e, ema_decay=DECAY if ema else 0.0)


def fresh(name):
    b = {k: x.to(DEV) for k, x in state_of(name).items()}
    b["shadow"] = torch.zeros_like(b["p"], dtype=torch.bfloat16)
    return b


def hyper_dev(kind):
    return torch.tensor([LR, BC1, BC2, 3.0] if kind == "lamb" else [LR, 0.0, 0.0, 0.0], dtype=torch.float32,
                        device=DEV)


def check(kind, name, bufs, ws, want, ema, mom=MOM):
    ns = len(ARENAS[name])
    trust = ws[0][:ns].cpu().double()
    sums = ws[0][ns:3 * ns].cpu().double().reshape(ns, 2)
    assert torch.allclose(sums, torch.tensor(want["sums"], dtype=torch.float64), rtol=RTOL, atol=0), "sums"
    assert torch.allclose(trust, torch.tensor(want["trust"], dtype=torch.float64), rtol=RTOL, atol=0), "trust"
    keys = ["p"] + (["m", "v"] if kind == "lamb" else (["vel"] if mom > 0 else [])) + (["ema"] if ema else [])
    for k in keys:
        assert torch.allclose(bufs[k].cpu().double(), want[k], **TOL), k
    if not ema:
        assert torch.equal(bufs["ema"].cpu(), state_of(name)["ema"])
    assert torch.equal(bufs["g"].cpu(), state_of(name)["g"])  # the gradient is never rewritten
    assert torch.equal(bufs["shadow"], bufs["p"].bfloat16())
    offs, counts, total, _ = layout(name)  # the gaps between the slices stay zero
    gap = torch.ones(total, dtype=torch.bool)
    for o, n in zip(offs, counts):
        gap[o:o + n] = False
    assert all((bufs[k].cpu()[gap] == 0).all() for k in keys)


@pytest.mark.parametrize("name", list(ARENAS))
@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_raw_step_against_float64(kind, name):
    from dcnn_amd.ops import hip
    t = make_tables(name)
    bufs, ws = fresh(name), hip.layerwise_workspace(t, torch.device(DEV))
    coef = torch.tensor([0.37], device=DEV)
    launch(kind, t, bufs, ws, coef, True, hyper_dev(kind))
    torch.cuda.synchronize()
    want = reference(kind, name, 0.37, True)
    assert any(abs(x - 1.0) > 0.05 for x in want["trust"])  # the ratios acted
    if len(ARENAS[name]) > 1:
        assert want["trust"][1] == 1.0 and ws[0][1].item() == 1.0  # a flagged segment
    check(kind, name, bufs, ws, want, True)


@pytest.mark.parametrize("coef,ema,hyper", list(itertools.product([False, True], repeat=3)))
@pytest.mark.parametrize("kind", ["lamb", "lars", "lars_nomomentum"])
def test_optional_inputs(kind, coef, ema, hyper):
    from dcnn_amd.ops import hip
    mom = 0.0 if kind == "lars_nomomentum" else MOM
    kind = kind.split("_")[0]
    t = make_tables("seven")
    bufs, ws = fresh("seven"), hip.layerwise_workspace(t, torch.device(DEV))
    c = torch.tensor([0.37], device=DEV) if coef else None
    launch(kind, t, bufs, ws, c, ema, hyper_dev(kind) if hyper else None, mom)
    torch.cuda.synchronize()
    check(kind, "seven", bufs, ws, reference(kind, "seven", 0.37 if coef else None, ema, mom), ema, mom)
    if mom == 0.0:
        assert torch.equal(bufs["vel"].cpu(), state_of("seven")["vel"])


@pytest.mark.parametrize("name", list(ARENAS))
@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_bit_reproducible_eager_and_captured(kind, name):
    """Twice eager on one stream, then five times inside one captured graph, replayed twice: all
    bit-identical. The ticket resets itself and the order depends on the table only."""
    from dcnn_amd.ops import hip
    t = make_tables(name)
    dev = torch.device(DEV)
    coef, hyper = torch.tensor([0.37], device=DEV), hyper_dev(kind)
    keys = ("p", "m", "v", "vel", "ema", "shadow")
    runs = [(fresh(name), hip.layerwise_workspace(t, dev)) for _ in range(2)]
    for bufs, ws in runs:
        launch(kind, t, bufs, ws, coef, True, hyper)
    torch.cuda.synchronize()
    (b0, w0), (b1, w1) = runs
    assert torch.equal(w0[0], w1[0]) and all(torch.equal(b0[k], b1[k]) for k in keys)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        hip.prewarm_tickets(dev, ("layerwise",))
        launch(kind, t, fresh(name), hip.layerwise_workspace(t, dev), coef, True, hyper)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    cap = [(fresh(name), hip.layerwise_workspace(t, dev)) for _ in range(5)]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        for bufs, ws in cap:
            launch(kind, t, bufs, ws, coef, True, hyper)
    for rep in range(2):
        for bufs, ws in cap:  # the same start for every replay
            for k, x in fresh(name).items():
                bufs[k].copy_(x)
            ws[0].fill_(-1.0)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        for i, (bufs, ws) in enumerate(cap):
            assert torch.equal(ws[0], w0[0]), (rep, i, "trust")
            assert all(torch.equal(bufs[k], b0[k]) for k in keys), (rep, i)


def test_host_checks_name_the_numbers():
    from dcnn_amd.ops import hip
    t = make_tables("seven")
    ws = hip.layerwise_workspace(t, torch.device(DEV))
    z = torch.zeros(t.cover - 64, device=DEV)
    with pytest.raises(ValueError, match=f"reaches element {t.cover}, the buffers hold {t.cover - 64}"):
        hip.lars_step(z, z.clone(), None, None, 0.1, 0.0, 0.0, 1e-3, 1e-8, t, *ws)
    z = torch.zeros(t.cover, device=DEV)
    with pytest.raises(ValueError, match="trust is a float32 GPU tensor of at least"):
        hip.lars_step(z, z.clone(), None, None, 0.1, 0.0, 0.0, 1e-3, 1e-8, t, ws[0][:3], ws[1])
    with pytest.raises(ValueError, match="ema_decay"):
        hip.lars_step(z, z.clone(), None, None, 0.1, 0.0, 0.0, 1e-3, 1e-8, t, *ws, ema=z.clone(), ema_decay=1.5)


# ---------------------------------------------------------------------------------------- models
@pytest.mark.parametrize("kind", KINDS)
def test_three_steps_match_the_formula_gpu(kind):
    m, opt = model_case(kind, "GPU:0")
    assert opt.fused() and opt._tables.chunks_dev.is_cuda and opt._trust.is_cuda


@pytest.mark.parametrize("kind", ["lamb_nodecay", "lars_nodecay"])
def test_raw_arena_gpu(kind):
    raw_case(kind, DEV)


@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_edge_cases_gpu(kind):
    edge_cases(kind, DEV)


def _net(kind):
    m, _, lf = _train_net()
    opt = make_opt(kind)
    opt.attach(m)
    return m, opt, lf


@pytest.mark.parametrize("kind", ["lamb_nodecay", "lars_nodecay"])
def test_captured_step_matches_eager(kind):
    """Three replays of the captured step leave the bits of three eager steps in the weights, the
    state and the trust table; the warm-up steps of the capture were rolled back."""
    from dcnn_amd.runtime.step import TrainStep
    torch.manual_seed(3)
    xs = [torch.randn(8, 3, 16, 16, device="cuda") for _ in range(3)]
    ys = [torch.randint(0, 10, (8,), device="cuda") for _ in range(3)]
    m, opt, lf = _net(kind)
    st = TrainStep(m, lf, opt, use_graph=False)
    m2, opt2, lf2 = _net(kind)
    st2 = TrainStep(m2, lf2, opt2, use_graph=True)
    init = m2.arena.data.clone()
    st2._capture(xs[0], ys[0])
    torch.cuda.synchronize()
    assert st2.graphs is not None and torch.equal(m2.arena.data, init)
    names = ("m", "v") if kind.startswith("lamb") else ("velocity",)
    assert all((getattr(opt2, n)[0] == 0).all() for n in names)
    for x, y in zip(xs, ys):
        st(x, y)
        st2(x, y)
        torch.cuda.synchronize()
        assert torch.equal(opt._trust, opt2._trust)
    assert torch.equal(m.arena.data, m2.arena.data) and not torch.equal(m.arena.data, init)
    assert all(torch.equal(getattr(opt, n)[0], getattr(opt2, n)[0]) for n in names)
    if kind.startswith("lamb"):
        assert opt.t == opt2.t == 3
    tr = opt.last_trust_ratios()
    flags = m.no_decay_flags()
    assert all(t == 1.0 for t, f in zip(tr, flags) if f) and any(t != 1.0 for t in tr)


def test_kernels_per_step(monkeypatch):
    """An Adam / SGD step launches exactly what it launched before LAMB and LARS existed (the library
    entry points of a step are counted); a LAMB step is its scalar update and lamb_step, a LARS step
    is lars_step."""
    from dcnn_amd.nn import SGD, Adam
    from dcnn_amd.ops._ext import kernels
    K = kernels()
    names = ("adam_scalars", "adam_step", "adam_step_nodecay", "adam_step_tail", "sgd_step", "sgd_step_tail",
             "grad_sumsq", "lamb_scalars", "lamb_step", "lars_step", "ema_swap", "cast_f32_bf16")
    calls = []

    def counted(name, fn):
        def wrapper(*a, **k):
            calls.append(name)
            return fn(*a, **k)
        return wrapper
    for n in names:
        monkeypatch.setattr(K, n, counted(n, getattr(K, n)))
    want = {"adam": ["adam_scalars", "adam_step"], "adamw_nodecay": ["adam_scalars", "adam_step_nodecay"],
            "sgd": ["sgd_step"], "lamb": ["lamb_scalars", "lamb_step"], "lars": ["lars_step"]}
    for kind, seq in want.items():
        m = _model("GPU:0")
        opt = {"adam": lambda: Adam(1e-3), "adamw_nodecay": lambda: Adam(1e-3, weight_decay=0.1,
                                                                          decouple_weight_decay=True,
                                                                          no_decay_norm_bias=True),
               "sgd": lambda: SGD(0.1, 0.9), "lamb": lambda: make_opt("lamb"), "lars": lambda: make_opt("lars")}[kind]()
        opt.attach(m)
        set_grads(m.gradients(), 1)
        opt.update()  # the first step uploads the scalars
        del calls[:]
        opt.update()
        torch.cuda.synchronize()
        assert calls == seq, (kind, calls)
