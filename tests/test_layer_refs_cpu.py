"""The float64 references of tests/layer_refs.py against torch autograd (where torch has the op) and
against the native CPU backend in float64, at the case lists the GPU tests use, within 1e-12 relative;
and the conditions the GPU tests rely on: no input on an activation or MAE / Huber kink by accident,
a clamped probability in the crossentropy case, a first-index rule in the tie cases."""
import pytest
import torch
import torch.nn.functional as F

import layer_refs as R
from layer_refs import BF16, F32, F64

RTOL = 1e-12
DTYPES = [F32, BF16]


def close(a, b, scale=None):
    """max|a - b| <= 1e-12 of the largest magnitude of b (``scale``: of the terms b is the difference
    of, where b itself cancels)."""
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    assert a.shape == b.shape
    s = max(float(b.abs().max()) if b.numel() else 0.0, scale or 0.0, 1e-300)
    err = float((a - b).abs().max()) if b.numel() else 0.0
    assert err <= RTOL * s, f"max error {err:.3e} against scale {s:.3e}"


def _gn_inputs(case, affine, seed=0):
    N, C, G, H, W = case
    g = torch.Generator().manual_seed(seed + 13 * C + H)
    x = torch.randn(N, C, H, W, generator=g, dtype=F64)
    dy = torch.randn(N, C, H, W, generator=g, dtype=F64)
    gamma = torch.rand(C, generator=g, dtype=F64) + 0.5 if affine else None
    beta = torch.randn(C, generator=g, dtype=F64) if affine else None
    return x, dy, gamma, beta


@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("case", R.GN_CASES, ids=str)
def test_groupnorm_reference(case, affine):
    from dcnn_amd.ops import cpu
    N, C, G, H, W = case
    x, dy, gamma, beta = _gn_inputs(case, affine)
    y, mean, istd = R.gn_fwd(x, G, gamma, beta)
    dx, dgamma, dbeta = R.gn_bwd(x, dy, G, gamma)
    # dx is a difference of terms of this size (a group of two elements cancels almost completely)
    dscale = float((istd.max() * dy.abs().max() * (gamma.abs().max() if affine else 1.0)))
    # torch autograd
    xt = x.clone().requires_grad_(True)
    gt = gamma.clone().requires_grad_(True) if affine else None
    bt = beta.clone().requires_grad_(True) if affine else None
    yt = F.group_norm(xt, G, gt, bt, R.GN_EPS)
    yt.backward(dy)
    close(y, yt.detach())
    close(dx, xt.grad, dscale)
    if affine:
        close(dgamma, gt.grad)
        close(dbeta, bt.grad)
    # the native CPU backend, its accumulation into dgamma / dbeta included
    yc, mc, ic = cpu.groupnorm_fwd(x, G, gamma, beta, R.GN_EPS)
    close(y, yc)
    close(mean, mc)
    close(istd, ic)
    pg, pb = torch.full((C,), 0.25, dtype=F64), torch.full((C,), -0.5, dtype=F64)
    ag, ab = pg.clone(), pb.clone()
    dxc = cpu.groupnorm_bwd(x, dy, G, gamma, mc, ic, ag, ab)
    close(dx, dxc, dscale)
    close(pg + dgamma, ag)
    close(pb + dbeta, ab)
    close(R.gn_var(x, G), 1.0 / istd ** 2 - R.GN_EPS, 1.0)


@pytest.mark.parametrize("case", R.POOL_CASES, ids=str)
def test_avgpool_reference(case):
    from dcnn_amd.ops import cpu
    N, C, H, W, ph, pw, sh, sw, pdh, pdw = case
    g = torch.Generator().manual_seed(C + H)
    x = torch.randn(N, C, H, W, generator=g, dtype=F64)
    y = R.avgpool_fwd(x, ph, pw, sh, sw, pdh, pdw)
    dy = torch.randn(y.shape, generator=g, dtype=F64)
    dx = R.avgpool_bwd(dy, H, W, ph, pw, sh, sw, pdh, pdw)
    assert tuple(y.shape[2:]) == R.pool_out(H, W, ph, pw, sh, sw, pdh, pdw)
    xt = x.clone().requires_grad_(True)
    yt = F.avg_pool2d(xt, (ph, pw), (sh, sw), (pdh, pdw), count_include_pad=True)
    yt.backward(dy)
    close(y, yt.detach())
    close(dx, xt.grad)
    close(y, cpu.avgpool_fwd(x, (ph, pw), (sh, sw), (pdh, pdw)))
    close(dx, cpu.avgpool_bwd(dy, (N, C, H, W), (ph, pw), (sh, sw), (pdh, pdw)))
    if sh > ph or sw > pw:  # stride > window: the skipped inputs get exactly nothing
        assert int((dx == 0).sum()) > 0
    for gcase in R.POOL_GLOBAL:
        d = R.distinct_dy(gcase[0], gcase[1], BF16)
        assert d.unique().numel() == d.numel() and torch.equal(d, R.distinct_dy(gcase[0], gcase[1], F32))


_TORCH_ACT = {"relu": lambda x, a: F.relu(x), "leaky_relu": lambda x, a: F.leaky_relu(x, a),
              "elu": lambda x, a: F.elu(x, a), "sigmoid": lambda x, a: torch.sigmoid(x),
              "tanh": lambda x, a: torch.tanh(x), "linear": lambda x, a: x * 1.0, "gelu": lambda x, a: F.gelu(x)}


@pytest.mark.parametrize("kind", R.ACT_KINDS)
def test_activation_reference(kind):
    from dcnn_amd.ops import cpu
    for alpha in R.act_alphas(kind):
        for n in R.ACT_NS:
            for dt in DTYPES:
                x, dy = R.act_inputs(n, dt)
                x, dy = x.double(), dy.double()
                y, dx = R.act_fwd(x, kind, alpha), dy * R.act_grad(x, kind, alpha)
                xt = x.clone().requires_grad_(True)
                yt = _TORCH_ACT[kind](xt, alpha)
                yt.backward(dy)
                # 1 - tanh^2, s (1 - s) and 1 + erf cancel: the terms are of size 1
                close(y, yt.detach(), 10.0 if kind == "gelu" else None)
                close(dx, xt.grad, float(dy.abs().max()) * (10.0 if kind == "gelu" else 1.0))
                close(y, cpu.act_fwd(x, kind, alpha), 10.0 if kind == "gelu" else None)
                close(dx, cpu.act_bwd(x, dy, kind, alpha), float(dy.abs().max()) * (10.0 if kind == "gelu" else 1.0))
                # at the exact zero the reference, torch and the CPU backend agree exactly
                z = x == 0
                assert int(z.sum()) == 1
                assert torch.equal(y[z], cpu.act_fwd(x, kind, alpha)[z])
                assert torch.equal(dx[z], cpu.act_bwd(x, dy, kind, alpha)[z])


def test_activation_inputs_avoid_the_kink():
    for n in R.ACT_NS:
        for dt in DTYPES:
            x, dy = R.act_inputs(n, dt)
            assert torch.equal(x, R.rounded(x, dt)) and torch.equal(dy, R.rounded(dy, dt))
            assert x[n // 2] == 0.0 and int((x == 0).sum()) == 1
            nz = x[x != 0]
            assert bool((nz.abs() > R.ACT_KINK).all()) and bool((x.abs() <= 10.0).all())
            if n >= 7:
                assert bool((x > 0).any()) and bool((x < 0).any())


def _softmax_inputs(shape, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return 3.0 * torch.randn(*shape, generator=g, dtype=F64), torch.randn(*shape, generator=g, dtype=F64)


@pytest.mark.parametrize("shape", R.SOFTMAX_CASES + [R.SOFTMAX_4D], ids=str)
def test_softmax_reference(shape):
    from dcnn_amd.ops import cpu
    x, dy = _softmax_inputs(shape)
    y = R.softmax_fwd(x)
    dx = R.softmax_bwd(y, dy)
    xt = x.clone().requires_grad_(True)
    yt = torch.softmax(xt, 1)
    yt.backward(dy)
    close(y, yt.detach())
    close(dx, xt.grad, float(dy.abs().max()))
    close(y, cpu.softmax_channels(x))
    close(dx, cpu.softmax_channels_bwd(y, dy), float(dy.abs().max()))
    close(y.sum(1), torch.ones_like(y.sum(1)))
    close(R.softmax_fwd(x + 1000.0), y, 1e4)  # shifted logits: the spacing of float64 at 1000 is 1e-13


def test_softmax_cases_cover_the_grid():
    rows = {r for r, _ in R.SOFTMAX_CASES}
    cs = {c for _, c in R.SOFTMAX_CASES}
    assert rows == {1, 3, 5, 257} and cs == {1, 10, 63, 64, 65, 200, 1000}
    assert {(5, 65), (257, 10), (1, 1000), (3, 1)} <= set(R.SOFTMAX_CASES)


def _torch_loss(kind, x, lab, t, param):
    """(loss, grad) by torch's own loss functions and autograd (one-hot targets)."""
    xt = x.clone().requires_grad_(True)
    if kind in ("softmax_crossentropy", "logsoftmax_crossentropy"):
        l = F.cross_entropy(xt, lab)
    elif kind == "crossentropy":  # the value only: the kernel's gradient (p - t) / N is not its derivative
        return F.nll_loss(torch.log(xt.detach().clamp(param, 1 - param)), lab), None
    elif kind == "mse":
        l = F.mse_loss(xt, t)
    elif kind == "mae":
        l = F.l1_loss(xt, t)
    else:
        l = F.huber_loss(xt, t, delta=param)
    l.backward()
    return l.detach(), xt.grad


@pytest.mark.parametrize("shape", R.LOSS_SHAPES, ids=str)
@pytest.mark.parametrize("kind", R.LOSS_KINDS)
def test_loss_reference(kind, shape):
    from dcnn_amd.ops import cpu
    N, C = shape
    for dt in DTYPES:
        x, lab, t, param = R.loss_case(kind, N, C, dt)
        x, t = x.double(), t.double()
        l, g, c = R.loss_ref(x, t, kind, param)
        lt, gt = _torch_loss(kind, x, lab, t, param)
        close(l, lt)
        if gt is not None:
            close(g, gt)
        else:
            close(g, (x - t) / N)
        for dense in (t, None):
            lc, gc, cc = cpu.loss_fused(x, dense, lab if dense is None else None, kind, param)
            close(l, lc)
            close(g, gc)
            assert int(c) == int(cc)
        # rows without a class above 0.5: no loss term, a full gradient
        xs, _, ts, _ = R.loss_case(kind, N, C, dt, soft=True)
        xs, ts = xs.double(), ts.double()
        assert bool((ts[1::3] <= 0.5).all()) and (kind in ("mse", "mae", "huber") or torch.equal(xs, x))
        ls, gs, cs = R.loss_ref(xs, ts, kind, param)
        lc, gc, cc = cpu.loss_fused(xs, ts, None, kind, param)
        close(ls, lc)
        close(gs, gc)
        assert int(cs) == int(cc)
        if kind in ("softmax_crossentropy", "logsoftmax_crossentropy", "crossentropy") and N > 1:
            keep = torch.ones(N, dtype=torch.bool)
            keep[1::3] = False
            lk, _, _ = R.loss_ref(x[keep], t[keep], kind, param)
            close(ls * N, lk * int(keep.sum()))
            assert bool((gs[~keep].abs().sum(1) > 0).all())
        # the gradient scale leaves the loss alone
        l2, g2, _ = R.loss_ref(x, t, kind, param, grad_scale=0.5)
        assert torch.equal(l2, l) and torch.equal(g2, g * 0.5)
        assert 0 < int(c) or N == 1


def test_loss_cases_avoid_the_kinks_and_reach_the_clamp():
    for N, C in R.LOSS_SHAPES:
        for dt in DTYPES:
            for kind in ("mae", "huber"):
                for soft in (False, True):
                    x, lab, tt, param = R.loss_case(kind, N, C, dt, soft)
                    assert torch.equal(x, R.rounded(x, dt))
                    d = (x.double() - tt.double()).abs()
                    assert bool((d > R.LOSS_KINK).all())
                    if kind == "huber":
                        assert bool(((d - param).abs() > R.LOSS_KINK).all())
                        assert bool((d < param).any()) and bool((d > param).any())
            x, lab, t, param = R.loss_case("crossentropy", N, C, dt)
            hot = x[torch.arange(N), lab]
            assert 0 < float(hot[0]) < param
            assert bool((x >= 0).all()) and bool((x <= 1).all())


@pytest.mark.parametrize("C,ties", R.TIE_SETS, ids=str)
def test_tie_cases_follow_the_first_index(C, ties):
    from dcnn_amd.ops import cpu
    assert {(200, (3, 67)), (200, (5, 6)), (200, (70, 130, 190))} <= set(R.TIE_SETS)
    for dt in DTYPES:
        x, lab = R.tie_case(C, ties, dt)
        top = x.max(1).values
        for k in range(C):
            assert bool((x[:, k] == top).all()) == (k in ties)
        assert torch.equal(R.first_argmax(x), torch.full((x.shape[0],), ties[0]))
        want = int((lab == ties[0]).sum())
        assert 0 < want < x.shape[0]
        # a rule that took another of the tied classes would count differently
        assert all(int((lab == k).sum()) != want for k in ties[1:])
        for kind in R.LOSS_KINDS:
            _, _, c = R.loss_ref(x.double(), R.one_hot(lab, C, F64), kind, R.LOSS_PARAM.get(kind, 0.0))
            _, _, cc = cpu.loss_fused(x.double(), None, lab, kind, R.LOSS_PARAM.get(kind, 0.0))
            assert int(c) == want == int(cc)
        # the target side: the target's maximum shared by ``ties``, a clear arg-max of the prediction
        xt, tt = R.tied_target_case(C, ties, dt)
        assert torch.equal(R.first_argmax(tt), torch.full((xt.shape[0],), ties[0]))
        win = R.first_argmax(xt)
        assert int((win == ties[0]).sum()) == 4 and all(int((win == k).sum()) != 4 for k in ties[1:])
        for kind in R.LOSS_KINDS:
            _, _, c = R.loss_ref(xt.double(), tt.double(), kind, R.LOSS_PARAM.get(kind, 0.0))
            _, _, cc = cpu.loss_fused(xt.double(), tt.double(), None, kind, R.LOSS_PARAM.get(kind, 0.0))
            assert int(c) == 4 == int(cc)


def test_noise_floor_is_the_float32_error_of_the_reference():
    x = torch.randn(7, 5, dtype=F64)
    assert R.noise_floor(lambda a: a * 2.0, x.float()) == (0.0,)  # exact in both
    e = R.noise_floor(lambda a: (a.sum().reshape(1), a * a), x)
    assert len(e) == 2 and all(0.0 <= v < 1e-5 for v in e) and max(e) > 0.0
    # integer tensors and plain numbers pass through unchanged
    lab = torch.tensor([1, 0])
    e = R.noise_floor(lambda p, t, k: R.loss_ref(p, R.one_hot(t, 3, p.dtype), k), torch.randn(2, 3), lab,
                      "softmax_crossentropy")
    assert len(e) == 3 and e[2] == 0.0
    assert R.tol32(torch.tensor([2.0, -4.0]), 1e-7) == 8e-7 + 4.0 * 2.0 ** -20
