"""The generic layer kernels on the GPU against the float64 references of tests/layer_refs.py, at the
edge shapes where each kernel takes another path: GroupNorm (norm.hip), average pool, activations,
channel softmax and dropout (pool_act.hip), the loss kinds 0..5 (loss_optim.hip) and the elementwise /
reduction / transpose family (ops.hip). tests/test_layer_refs_cpu.py checks the references themselves.

The tolerances are the rules of layer_refs.py (derived from the number formats and the reference's own
float32 error, never from a kernel's result); every figure is printed before it is asserted, and
profiles/layer_kernel_tests.md records one run's noise floors and worst errors."""
import pytest
import torch

import layer_refs as R
from layer_refs import BF16, CL, F32, F64

pytestmark = pytest.mark.gpu

DTYPES = [F32, BF16]
DT_IDS = ["f32", "bf16"]


class Checks:
    """Collects the comparisons of one test: every figure is printed, ``done`` fails on the misses."""

    def __init__(self, group):
        self.group, self.bad = group, []

    def close(self, name, got, ref, tol, e32=0.0):
        err, ratio = R.worst(got, ref, tol)
        print(f"[layer-kernels] {self.group} | {name} | e32 {e32:.3e} | err {err:.3e} | err/tol {ratio:.4f}")
        if not ratio <= 1.0:
            self.bad.append(f"{name}: err {err:.3e} is {ratio:.2f} x the bound (e32 {e32:.3e})")

    def out(self, name, got, ref, e32, dt):
        """a result in the compute dtype: the fp32 rule, plus one bf16 ulp for bf16"""
        ref = ref.double()
        self.close(name, got, ref, R.tol_bf16(ref, e32) if dt == BF16 else R.tol32(ref, e32), e32)

    def f32(self, name, got, ref, e32):
        """an fp32 result (the caller checks the device tensor's dtype): the fp32 rule"""
        self.close(name, got, ref.double(), R.tol32(ref.double(), e32), e32)

    def true(self, name, ok):
        if not ok:
            self.bad.append(name)

    def done(self):
        assert not self.bad, "; ".join(self.bad)


def dev(t, dt=None, cl=False):
    t = t.to(dt) if dt is not None else t
    t = t.cuda()
    return t.contiguous(memory_format=CL) if cl else t.contiguous()


def host(t):
    return t.detach().float().cpu() if t.is_floating_point() else t.detach().cpu()


# ------------------------------------------------------------------------------ GroupNorm
def _gn_case(case, dt, affine, mean=0.0):
    N, C, G, H, W = case
    g = torch.Generator().manual_seed(N + 13 * C + 7 * G + H)
    x = R.rounded(mean + torch.randn(N, C, H, W, generator=g), dt)
    dy = R.rounded(torch.randn(N, C, H, W, generator=g), dt)
    gamma = torch.rand(C, generator=g) + 0.5 if affine else None
    beta = torch.randn(C, generator=g) if affine else None
    pre = (torch.randn(C, generator=g), torch.randn(C, generator=g)) if affine else (None, None)
    return x, dy, gamma, beta, pre


@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", R.GN_CASES, ids=str)
def test_groupnorm(case, dt, affine):
    from dcnn_amd.ops import hip
    N, C, G, H, W = case
    x, dy, gamma, beta, (pg, pb) = _gn_case(case, dt, affine)
    ck = Checks(f"groupnorm {DT_IDS[DTYPES.index(dt)]}")
    xg, dyg = dev(x, dt, True), dev(dy, dt, True)
    gg, bg = (dev(gamma), dev(beta)) if affine else (None, None)

    def run():
        y, mean, istd = hip.gn_fwd(xg, G, gg, bg, R.GN_EPS)
        dg, db = (dev(pg), dev(pb)) if affine else (None, None)
        dx = hip.gn_bwd(dyg, xg, G, gg, mean, istd, dg, db)
        torch.cuda.synchronize()
        return y, mean, istd, dx, dg, db

    y, mean, istd, dx, dg, db = run()
    ry, rmean, ristd = R.evaluate(R.gn_fwd, F64, x, G, gamma, beta)
    ey, emean, eistd = R.noise_floor(R.gn_fwd, x, G, gamma, beta)
    rdx, rdg, rdb = R.evaluate(R.gn_bwd, F64, x, dy, G, gamma)
    edx, edg, edb = R.noise_floor(R.gn_bwd, x, dy, G, gamma)
    assert y.dtype == dt and dx.dtype == dt and y.shape == x.shape and mean.shape == (N * G,)
    assert mean.dtype == F32 and istd.dtype == F32 and (not affine or (dg.dtype == F32 and db.dtype == F32))
    ck.out(f"{case} y", host(y), ry, ey, dt)
    ck.f32(f"{case} mean", host(mean), rmean, emean)
    ck.f32(f"{case} istd", host(istd), ristd, eistd)
    ck.out(f"{case} dx", host(dx), rdx, edx, dt)
    if affine:  # accumulated: prefill plus the reference
        ck.f32(f"{case} dgamma", host(dg), pg.double() + rdg, edg)
        ck.f32(f"{case} dbeta", host(db), pb.double() + rdb, edb)
    # fixed summation order: a second call gives the same bits
    for name, a, b in zip(("y", "mean", "istd", "dx", "dgamma", "dbeta"), (y, mean, istd, dx, dg, db), run()):
        ck.true(f"{case} {name} differs between two calls", a is None or torch.equal(a, b))
    ck.done()


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_groupnorm_large_mean(dt):
    """x = 1000 + noise: the centred second pass keeps the variance (E[x^2] - mean^2 would lose it)."""
    from dcnn_amd.ops import hip
    case = R.GN_LARGE_MEAN
    N, C, G, H, W = case
    x, _, gamma, beta, _ = _gn_case(case, dt, True, mean=1000.0)
    ck = Checks(f"groupnorm large mean {DT_IDS[DTYPES.index(dt)]}")
    y, mean, istd = hip.gn_fwd(dev(x, dt, True), G, dev(gamma), dev(beta), R.GN_EPS)
    torch.cuda.synchronize()
    ry, rmean, _ = R.evaluate(R.gn_fwd, F64, x, G, gamma, beta)
    ey, emean, _ = R.noise_floor(R.gn_fwd, x, G, gamma, beta)
    (rvar,), (evar,) = R.evaluate(R.gn_var, F64, x, G), R.noise_floor(R.gn_var, x, G)
    assert float(rvar.min()) > 0.5
    assert mean.dtype == F32 and istd.dtype == F32 and y.dtype == dt
    var = 1.0 / host(istd).double() ** 2 - R.GN_EPS
    ck.close(f"{case} var", var, rvar, R.tol32(rvar, evar), evar)
    ck.f32(f"{case} mean", host(mean), rmean, emean)
    ck.out(f"{case} y", host(y), ry, ey, dt)
    ck.done()


# ------------------------------------------------------------------------------ average pool
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", R.POOL_CASES, ids=str)
def test_avgpool(case, dt):
    from dcnn_amd.ops import hip
    N, C, H, W, ph, pw, sh, sw, pdh, pdw = case
    geo = (ph, pw, sh, sw, pdh, pdw)
    g = torch.Generator().manual_seed(C + 3 * H + ph)
    x = R.rounded(torch.randn(N, C, H, W, generator=g), dt)
    OH, OW = R.pool_out(H, W, *geo)
    if case in R.POOL_GLOBAL:  # a distinct value per (n, c): an index mix-up cannot cancel
        dy = R.distinct_dy(N, C, dt)
    else:
        dy = R.rounded(torch.randn(N, C, OH, OW, generator=g), dt)
    ck = Checks(f"avgpool {DT_IDS[DTYPES.index(dt)]}")
    y = hip.avgpool_fwd(dev(x, dt, True), *geo)
    dx = hip.avgpool_bwd(dev(dy, dt, True), (N, C, H, W), *geo)
    torch.cuda.synchronize()
    assert y.dtype == dt and tuple(y.shape) == (N, C, OH, OW) and dx.dtype == dt and tuple(dx.shape) == (N, C, H, W)
    (ry,), (ey,) = R.evaluate(R.avgpool_fwd, F64, x, *geo), R.noise_floor(R.avgpool_fwd, x, *geo)
    (rdx,), (edx,) = R.evaluate(R.avgpool_bwd, F64, dy, H, W, *geo), R.noise_floor(R.avgpool_bwd, dy, H, W, *geo)
    ck.out(f"{case} y", host(y), ry, ey, dt)
    ck.out(f"{case} dx", host(dx), rdx, edx, dt)
    # inputs no window covers get exactly zero
    (reach,) = R.evaluate(R.avgpool_bwd, F64, torch.ones(N, C, OH, OW), H, W, *geo)
    if sh > ph or sw > pw:
        assert int((reach == 0).sum()) > 0
    ck.true(f"{case} uncovered inputs are not exactly zero", torch.equal(host(dx)[reach == 0], torch.zeros(int((reach == 0).sum()))))
    ck.done()


# ------------------------------------------------------------------------------ activations
def _f32(v):
    return float(torch.tensor(v, dtype=F32))


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kind", R.ACT_KINDS)
def test_activation(kind, dt):
    from dcnn_amd.ops import cpu, hip
    bf = dt == BF16
    ck = Checks(f"activation {DT_IDS[DTYPES.index(dt)]}")
    for alpha in map(_f32, R.act_alphas(kind)):  # the kernel receives alpha as a float32
        for n in R.ACT_NS:
            x, dy = R.act_inputs(n, dt)
            xg, dyg = dev(x, dt), dev(dy, dt)
            y, dx = hip.act_fwd(xg, kind, alpha), hip.act_bwd(xg, dyg, kind, alpha)
            torch.cuda.synchronize()
            assert y.dtype == dt and dx.dtype == dt and y.shape == x.shape and dx.shape == x.shape
            ry = R.act_fwd(x.double(), kind, alpha)
            rdx = dy.double() * R.act_grad(x.double(), kind, alpha)
            tag = f"{kind} alpha {alpha:g} n {n}"
            ck.close(f"{tag} y", host(y), ry, R.tol_fast(ry, bf))
            ck.close(f"{tag} dx", host(dx), rdx, R.tol_fast(rdx, bf))
            # at the exact zero both devices agree exactly
            z = x == 0
            cy, cdx = cpu.act_fwd(x, kind, alpha), cpu.act_bwd(x, dy, kind, alpha)
            ck.true(f"{tag}: y(0) = {host(y)[z].tolist()}, the CPU backend gives {cy[z].tolist()}",
                    torch.equal(host(y)[z], R.rounded(cy[z], dt)))
            ck.true(f"{tag}: dx(0) = {host(dx)[z].tolist()}, the CPU backend gives {cdx[z].tolist()}",
                    torch.equal(host(dx)[z], R.rounded(cdx[z], dt)))
    ck.done()


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kind", R.ACT_KINDS)
def test_activation_saturates(kind, dt):
    """+-20, +-88, +-1e-30: finite results at the saturated value (no tight bound: __expf is a fast
    intrinsic), forward and derivative."""
    from dcnn_amd.ops import hip
    ck = Checks(f"activation saturating {DT_IDS[DTYPES.index(dt)]}")
    x = R.rounded(torch.tensor(R.ACT_SATURATING), dt)
    for alpha in map(_f32, R.act_alphas(kind)):
        xg = dev(x, dt)
        y, dx = hip.act_fwd(xg, kind, alpha), hip.act_bwd(xg, torch.ones_like(xg), kind, alpha)
        torch.cuda.synchronize()
        ry, rdx = R.act_fwd(x.double(), kind, alpha), R.act_grad(x.double(), kind, alpha)
        ck.true(f"{kind} {alpha:g}: not finite: y {host(y).tolist()} dx {host(dx).tolist()}",
                bool(torch.isfinite(host(y)).all()) and bool(torch.isfinite(host(dx)).all()))
        loose = lambda r: 1e-3 * r.abs() + 1e-6 + (2.0 ** -8 * r.abs() if dt == BF16 else 0.0)
        ck.close(f"{kind} alpha {alpha:g} y", host(y), ry, loose(ry))
        ck.close(f"{kind} alpha {alpha:g} dx", host(dx), rdx, loose(rdx))
    ck.done()


# ------------------------------------------------------------------------------ softmax
def _softmax_check(ck, tag, x, dy, dt, cl=False):
    from dcnn_amd.ops import hip
    bf = dt == BF16
    C = x.shape[1]
    y = hip.softmax_channels(dev(x, dt, cl))
    ry = R.softmax_fwd(x.double())
    yin = R.rounded(ry, dt)  # the backward's input: the rounded reference output
    dx = hip.softmax_channels_bwd(dev(yin, dt, cl), dev(dy, dt, cl))
    torch.cuda.synchronize()
    assert y.dtype == dt and y.shape == x.shape and dx.dtype == dt and dx.shape == x.shape
    rdx = R.softmax_bwd(yin.double(), dy.double())
    ck.close(f"{tag} y", host(y), ry, R.tol_fast(ry, bf))
    one = torch.ones(x.numel() // C, dtype=F64)
    ck.close(f"{tag} row sums", host(y).double().sum(1).reshape(-1), one, R.tol_fast(one, bf))
    ck.close(f"{tag} dx", host(dx), rdx, R.tol_fast(rdx, bf))


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", R.SOFTMAX_CASES + [R.SOFTMAX_4D], ids=str)
def test_softmax(shape, dt):
    g = torch.Generator().manual_seed(sum(shape))
    x = R.rounded(3.0 * torch.randn(*shape, generator=g), dt)
    dy = R.rounded(torch.randn(*shape, generator=g), dt)
    ck = Checks(f"softmax {DT_IDS[DTYPES.index(dt)]}")
    _softmax_check(ck, f"{shape}", x, dy, dt, cl=len(shape) == 4)
    ck.done()


def test_softmax_shifted_logits():
    g = torch.Generator().manual_seed(5)
    x = R.rounded(1000.0 + 3.0 * torch.randn(5, 65, generator=g), F32)
    ck = Checks("softmax f32")
    _softmax_check(ck, "(5, 65) + 1000", x, torch.randn(5, 65, generator=g), F32)
    ck.done()


# ------------------------------------------------------------------------------ loss kinds 0..5
def _loss_check(ck, tag, out, x, t, kind, param, dt, scale=1.0):
    loss, grad, correct = out
    rl, rg, rc = R.evaluate(R.loss_ref, F64, x, t, kind, param, scale)
    el, eg, _ = R.noise_floor(R.loss_ref, x, t, kind, param, scale)
    assert loss.dtype == F32 and grad.dtype == dt and tuple(grad.shape) == tuple(x.shape)
    ck.f32(f"{tag} loss", host(loss), rl, el)
    ck.out(f"{tag} grad", host(grad), rg, eg, dt)
    ck.true(f"{tag}: correct {int(correct)} != {int(rc)}", int(correct) == int(rc))


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", R.LOSS_SHAPES, ids=str)
@pytest.mark.parametrize("kind", R.LOSS_KINDS)
def test_loss(kind, shape, dt):
    from dcnn_amd.ops import hip
    N, C = shape
    x, lab, t, param = R.loss_case(kind, N, C, dt)
    ck = Checks(f"loss {DT_IDS[DTYPES.index(dt)]}")
    xg, tg, lg = dev(x, dt), dev(t), lab.cuda()
    dense = hip.loss_fused(xg, tg, None, kind, param)
    label = hip.loss_fused(xg, None, lg, kind, param)
    half = hip.loss_fused(xg, tg, None, kind, param, True, 0.5)
    nograd = hip.loss_fused(xg, tg, None, kind, param, False)
    torch.cuda.synchronize()
    tag = f"{kind} {shape}"
    _loss_check(ck, tag, dense, x, t, kind, param, dt)
    for name, a, b in zip(("loss", "grad", "correct"), dense, label):
        ck.true(f"{tag}: labels and the one-hot target give different {name} bits", torch.equal(a, b))
    # grad_scale: the loss and the count are unchanged, the gradient is scaled (0.5: exactly)
    _loss_check(ck, f"{tag} grad_scale 0.5", half, x, t, kind, param, dt, 0.5)
    ck.true(f"{tag}: grad_scale changed the loss or the count",
            torch.equal(half[0], dense[0]) and torch.equal(half[2], dense[2]))
    ck.true(f"{tag}: grad_scale 0.5 is not half the gradient", torch.equal(half[1], dense[1] * 0.5))
    ck.true(f"{tag}: want_grad=False changed the loss or the count",
            nograd[1] is None and torch.equal(nograd[0], dense[0]) and torch.equal(nograd[2], dense[2]))
    # rows without a class above 0.5: no loss term, a full gradient
    xs, _, ts, _ = R.loss_case(kind, N, C, dt, soft=True)
    soft = hip.loss_fused(dev(xs, dt), dev(ts), None, kind, param)
    torch.cuda.synchronize()
    _loss_check(ck, f"{tag} soft rows", soft, xs, ts, kind, param, dt)
    ck.done()


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("C,ties", R.TIE_SETS, ids=str)
def test_loss_argmax_ties_take_the_first_index(C, ties, dt):
    from dcnn_amd.ops import hip
    x, lab = R.tie_case(C, ties, dt)
    want = int((lab == ties[0]).sum())
    ck = Checks("loss ties")
    for kind in R.LOSS_KINDS:
        param = R.LOSS_PARAM.get(kind, 0.0)
        _, _, rc = R.loss_ref(x.double(), R.one_hot(lab, C, F64), kind, param)
        assert int(rc) == want
        a = hip.loss_fused(dev(x, dt), None, lab.cuda(), kind, param)
        b = hip.loss_fused(dev(x, dt), dev(R.one_hot(lab, C)), None, kind, param, False)
        torch.cuda.synchronize()
        ck.true(f"{kind} C {C} ties {ties}: correct {int(a[2])} / {int(b[2])}, the first-index rule gives {want}",
                int(a[2]) == want and int(b[2]) == want)
    # the same rule on the target side: a dense target whose maximum is shared by ``ties``
    xt, tt = R.tied_target_case(C, ties, dt)
    for kind in R.LOSS_KINDS:
        param = R.LOSS_PARAM.get(kind, 0.0)
        _, _, rc = R.loss_ref(xt.double(), tt.double(), kind, param)
        assert int(rc) == 4
        c = hip.loss_fused(dev(xt, dt), dev(tt), None, kind, param, False)[2]
        torch.cuda.synchronize()
        ck.true(f"{kind} C {C} tied target {ties}: correct {int(c)}, the first-index rule gives 4", int(c) == 4)
    ck.done()


@pytest.mark.parametrize("kind", ["softmax_crossentropy", "mse"])
def test_loss_ticket_resets_between_calls(kind):
    """N = 5, 257, 5 back to back on one stream: each equals its stand-alone bits."""
    from dcnn_amd.ops import hip
    cases = [R.loss_case(kind, N, 10, F32) for N in (5, 257, 5)]
    args = [(dev(x), dev(t), None, kind, param) for x, _, t, param in cases]
    alone = []
    for a in args:
        alone.append(hip.loss_fused(*a))
        torch.cuda.synchronize()
    chain = [hip.loss_fused(*a) for a in args]
    torch.cuda.synchronize()
    for N, u, v in zip((5, 257, 5), alone, chain):
        for name, p, q in zip(("loss", "grad", "correct"), u, v):
            assert torch.equal(p, q), f"N {N}: {name} differs in the chain"
    assert torch.equal(alone[0][0], alone[2][0])


@pytest.mark.parametrize("kind", R.LOSS_KINDS)
def test_loss_layer_gives_the_kernel_bits(kind):
    """Loss.loss_and_grad ([N, C, 1, 1] predictions, labels or dense targets) is hip.loss_fused."""
    from dcnn_amd.nn.loss import LossFactory
    from dcnn_amd.ops import hip
    L = LossFactory.create(kind)
    x, lab, t, _ = R.loss_case(kind, 5, 63, F32)
    xg = dev(x)
    want = hip.loss_fused(xg, dev(t), None, kind, L.param, True, 0.5)
    for tgt in (t.cuda(), lab.cuda(), t.view(5, 63, 1, 1).cuda()):
        got = L.loss_and_grad(xg.view(5, 63, 1, 1), tgt, grad_scale=0.5)
        torch.cuda.synchronize()
        assert torch.equal(got[0].reshape(-1), want[0]) and torch.equal(got[2].reshape(-1), want[2])
        assert torch.equal(got[1].reshape(5, 63), want[1])


# ------------------------------------------------------------------------------ generic ops (ops.hip)
EW_NS = [1, 3, 4, 5, 1023]
# element offsets of (a, b, out) inside their 16-byte aligned buffers: out at 4 is aligned
EW_ALIGN = {"aligned": (0, 0, 4), "a+1": (1, 0, 4), "out+1": (0, 0, 5), "b+2": (0, 2, 4)}
GUARD = -12345.0
_BIN = {"add": lambda a, b: a + b, "sub": lambda a, b: a - b, "mul": lambda a, b: a * b, "div": lambda a, b: a / b,
        "min": torch.minimum, "max": torch.maximum, "equal": lambda a, b: (a == b).to(a.dtype),
        "greater": lambda a, b: (a > b).to(a.dtype)}
_SCALAR = {"add_scalar": lambda a, s: a + s, "sub_scalar": lambda a, s: a - s, "mul_scalar": lambda a, s: a * s,
           "div_scalar": lambda a, s: a / s, "scalar_max": lambda a, s: a.clamp(min=s)}
_UNARY = {"sqrt": torch.sqrt, "rsqrt": torch.rsqrt, "rcp": torch.reciprocal, "abs": torch.abs, "exp": torch.exp,
          "log": torch.log, "copy": torch.clone}
_UNARY2 = {"clamp": lambda a, lo, hi: a.clamp(lo, hi), "sub_mul_scalar": lambda a, s, m: (a - s) * m,
           "mul_add_scalar": lambda a, m, s: a * m + s}
_TERNARY = {"fmadd": lambda a, b, c: a * b + c, "fmsub": lambda a, b, c: a * b - c, "fnmadd": lambda a, b, c: c - a * b}


def _view(t, off):
    """t as a contiguous device view at element offset ``off`` of a fresh (16-byte aligned) buffer."""
    buf = torch.full((t.numel() + 8,), GUARD, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + t.numel()]
    v.copy_(t)
    return buf, v


def _guards_ok(buf, off, n):
    b = buf.cpu()
    return bool((b[:off] == GUARD).all()) and bool((b[off + n:] == GUARD).all())


@pytest.mark.parametrize("align", list(EW_ALIGN), ids=list(EW_ALIGN))
@pytest.mark.parametrize("n", EW_NS)
def test_elementwise(n, align):
    from dcnn_amd.ops import generic as G
    ao, bo, oo = EW_ALIGN[align]
    g = torch.Generator().manual_seed(n)
    a = torch.randn(n, generator=g)
    b = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0) * (0.5 + torch.rand(n, generator=g))
    b[::2] = a[::2] if n > 1 else b[::2]  # equal elements for equal / greater / min / max
    b = torch.where(b == 0, torch.ones_like(b), b)
    pos = 0.1 + 3.0 * torch.rand(n, generator=g)  # sqrt / rsqrt / rcp / log take positive inputs
    c = torch.randn(n, generator=g)
    s, s2 = _f32(0.7), _f32(-1.3)
    ck = Checks("elementwise")

    def run(name, fn, ref, ins, scalars=(), acc=None):
        """out = fn(*ins, *scalars[, out]) on views at the case's offsets; ``acc``: the in-place operand."""
        views = [_view(t, o)[1] for t, o in zip(ins, (ao, bo))]
        obuf, out = _view(acc if acc is not None else torch.full((n,), GUARD), oo)
        assert (views[0].data_ptr() % 16 == 0) == (ao == 0) and (out.data_ptr() % 16 == 0) == (oo == 4)
        res = fn(*views, *scalars, out)
        torch.cuda.synchronize()
        assert res.data_ptr() == out.data_ptr()
        full = list(ins) + ([acc] if acc is not None else [])
        (r,), (e,) = R.evaluate(ref, F64, *full, *scalars), R.noise_floor(ref, *full, *scalars)
        assert out.dtype == F32
        ck.f32(f"{name} n {n} {align}", host(out), r, e)
        if name in ("exp", "log"):  # __expf / __logf: the small elements as well, relative (on top of the rule)
            ck.close(f"{name} n {n} {align} relative", host(out), r, R.tol_fast(r, False))
        ck.true(f"{name} n {n} {align}: wrote outside its {n} elements", _guards_ok(obuf, oo, n))

    for name, ref in _BIN.items():
        run(name, lambda x, y, o, f=getattr(G, name): f(x, y, o), ref, (a, b))
    for name, ref in _SCALAR.items():
        run(name, lambda x, v, o, f=getattr(G, name): f(x, v, o), ref, (a,), (s,))
    for name, ref in _UNARY.items():
        src = a if name in ("abs", "exp", "copy") else pos
        run(name, lambda x, o, f=getattr(G, name): f(x, o), ref, (src,))
    run("clamp", lambda x, lo, hi, o: G.clamp(x, lo, hi, o), _UNARY2["clamp"], (a,), (s2, s))
    run("sub_mul_scalar", lambda x, u, v, o: G.sub_mul_scalar(x, u, v, o), _UNARY2["sub_mul_scalar"], (a,), (s, s2))
    run("mul_add_scalar", lambda x, u, v, o: G.mul_add_scalar(x, u, v, o), _UNARY2["mul_add_scalar"], (a,), (s, s2))
    # in place on the accumulator (at the out offset: "out+1" misaligns it)
    for name, ref in _TERNARY.items():
        run(name, lambda x, y, o, f=getattr(G, name): f(x, y, o), ref, (a, b), acc=c)
    run("axpy", lambda x, v, o: G.axpy(v, x, o), lambda x, y, v: y + v * x, (a,), (s,), acc=c)
    ck.done()


@pytest.mark.parametrize("n", [1, 63, 255, 257])
def test_reductions(n):
    from dcnn_amd.ops import generic as G
    g = torch.Generator().manual_seed(n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    big = R.rounded(1e4 + torch.randn(n, generator=g), F32)
    big2 = R.rounded(big + torch.randn(n, generator=g), F32)
    ck = Checks("reductions")
    cases = [("sum", G.sum, lambda x: x.sum().reshape(1), (a,)),
             ("dot_product", G.dot_product, lambda x, y: (x * y).sum().reshape(1), (a, b)),
             ("norm_squared", G.norm_squared, lambda x: (x * x).sum().reshape(1), (a,)),
             ("sum_squared_diff", G.sum_squared_diff, lambda x, y: ((x - y) ** 2).sum().reshape(1), (a, b)),
             ("sum_squared_diff near 1e4", G.sum_squared_diff, lambda x, y: ((x - y) ** 2).sum().reshape(1), (big, big2))]
    for name, fn, ref, ins in cases:
        got = fn(*[dev(t) for t in ins])
        torch.cuda.synchronize()
        assert got.dtype == F32 and got.numel() == 1
        (r,), (e,) = R.evaluate(ref, F64, *ins), R.noise_floor(ref, *ins)
        ck.f32(f"{name} n {n}", host(got), r, e)
    ck.done()


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 5, 70), (3, 65, 64), (1, 130, 3)], ids=str)
def test_bf16_batched_transpose(shape):
    """transpose16_kernel through hip.nchw_nhwc (the bf16 Flatten path), both directions: bit-exact."""
    from dcnn_amd.ops import hip
    batch, rows, cols = shape
    g = torch.Generator().manual_seed(rows + cols)
    m = torch.randn(batch, rows, cols, generator=g).to(BF16)
    want = m.transpose(1, 2).contiguous()  # [batch][cols][rows]
    # NCHW -> NHWC: per image [C = rows][HW = cols] -> [HW][C]
    y = hip.nchw_nhwc(m.view(batch, rows, cols, 1).cuda(), True)
    torch.cuda.synchronize()
    assert y.dtype == BF16 and tuple(y.shape) == (batch, rows, cols, 1) and y.is_contiguous(memory_format=CL)
    assert torch.equal(y.permute(0, 2, 3, 1).reshape(batch, cols, rows).cpu(), want)
    # NHWC -> NCHW: per image [HW = rows][C = cols] -> [C][HW]
    x = m.view(batch, rows, 1, cols).permute(0, 3, 1, 2).cuda()  # logical (batch, C = cols, H = rows, 1), NHWC memory
    assert x.is_contiguous(memory_format=CL)
    z = hip.nchw_nhwc(x, False)
    torch.cuda.synchronize()
    assert z.dtype == BF16 and tuple(z.shape) == (batch, cols, rows, 1) and z.is_contiguous()
    assert torch.equal(z.reshape(batch, cols, rows).cpu(), want)


# ------------------------------------------------------------------------------ dropout
def _dropout(n, p, dt, seed=1234):
    from dcnn_amd.ops import hip
    g = torch.Generator().manual_seed(n)
    x = R.rounded(1.0 + torch.rand(n, generator=g), dt)  # no zeros: y != 0 is the mask
    y = hip.dropout(dev(x, dt), p, seed)
    torch.cuda.synchronize()
    assert y.dtype == dt and y.shape == x.shape
    return x, host(y)


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("n", [1, 5, 1003])
def test_dropout(n, p):
    x, y = _dropout(n, p, F32)
    keep = y != 0
    # Dropped values are exactly 0. Kept values are x / (1 - p) as inverted dropout forms it, here and in
    # the project this one was modelled on: the scale is taken once as the float32 reciprocal 1 / (1 - p)
    # and multiplied in, so the expected bits are x * fl32(1 / (1 - p)). That product can differ from the
    # single float32 division x / (1 - p) in the last bit (two roundings instead of one), never by more.
    one_minus_p = torch.ones(1) - torch.tensor(p, dtype=F32)
    scale = torch.ones(1) / one_minus_p
    assert torch.equal(y, torch.where(keep, x * scale, torch.zeros_like(x)))
    div = x / one_minus_p
    assert bool(((y - div).abs()[keep] <= 2.0 ** -23 * div.abs()[keep]).all())
    xb, yb = _dropout(n, p, BF16)
    assert torch.equal(yb != 0, keep), "the bf16 and fp32 masks of one seed differ"
    assert torch.equal(yb[keep], R.rounded(xb[keep] * scale, BF16))
    if p == 0.0:
        assert bool(keep.all()) and torch.equal(y, x)
    if n == 1003:  # counter-based draw: element i does not depend on n
        _, y5 = _dropout(5, p, F32)
        assert torch.equal(y5 != 0, keep[:5])
        if p > 0:  # 1003 draws of a Bernoulli(0.7): mean 702, sigma 14.5; 4.5 sigma
            assert 637 <= int(keep.sum()) <= 767
            _, other = _dropout(n, p, F32, seed=99)
            assert not torch.equal(other != 0, keep)
