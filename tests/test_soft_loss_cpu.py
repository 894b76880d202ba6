"""Soft-target cross entropy with label smoothing on the native CPU backend (``soft_crossentropy``,
csrc/native/cpu_ops.cpp loss_fused kind 5) against the float64 formulas written out with
``log_softmax``:

    t' = (1 - eps) t + eps / C,  S = sum_c t',  loss = mean_n(S lse - sum_c t' x),
    grad = grad_scale / N (S softmax(x) - t'),  hit = argmax x == argmax t (first maximum wins).

Tolerance: rtol 1e-5, atol 1e-7, the one tests/test_cpp_host_blocks.py uses for this backend."""
import pytest
import torch

from dcnn_amd.nn import LossFactory, SoftmaxCrossEntropyLoss, SoftTargetCrossEntropyLoss
from dcnn_amd.nn.loss import LossConfig

TOL = dict(rtol=1e-5, atol=1e-7)


def _inputs(N, C, dense, dtype, seed=0):
    g = torch.Generator().manual_seed(1000 * N + C + seed)
    x = (3.0 * torch.randn(N, C, generator=g, dtype=torch.float64)).to(dtype)
    lab = torch.randint(0, C, (N,), generator=g)
    if not dense:
        return x, lab, torch.nn.functional.one_hot(lab, C).double()
    # a mixed target: lam on one class, 1 - lam on another (sometimes the same one)
    lam = torch.rand(N, generator=g, dtype=torch.float64)
    other = torch.randint(0, C, (N,), generator=g)
    t = torch.zeros(N, C, dtype=torch.float64)
    t[torch.arange(N), lab] += lam
    t[torch.arange(N), other] += 1 - lam
    t = t.float()  # the mixer's targets are float32
    return x, t, t.double()


def _formula(x, t64, eps, grad_scale=1.0):
    N, C = x.shape
    ts = (1 - eps) * t64 + eps / C
    lsm = torch.log_softmax(x.double(), 1)
    lse = x.double()[:, :1] - lsm[:, :1]
    S = ts.sum(1, keepdim=True)
    loss = (S * lse - (ts * x.double()).sum(1, keepdim=True)).sum() / N
    grad = grad_scale / N * (S * lsm.exp() - ts)
    hits = int((x.argmax(1) == t64.argmax(1)).sum())
    return loss, grad, hits


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("dense", [True, False], ids=["dense", "labels"])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("C", [3, 10, 200, 1000])
@pytest.mark.parametrize("N", [1, 5, 64])
def test_native_kind_matches_the_formulas(N, C, eps, dense, dtype):
    x, tgt, t64 = _inputs(N, C, dense, dtype)
    loss, grad, correct = LossFactory.create("soft_crossentropy", label_smoothing=eps).loss_and_grad(x, tgt)
    rl, rg, rh = _formula(x, t64, eps)
    assert loss.dtype == dtype and grad.dtype == dtype and grad.shape == x.shape
    assert torch.allclose(loss.double().reshape(()), rl, **TOL), (float(loss), float(rl))
    assert torch.allclose(grad.double(), rg, **TOL), float((grad.double() - rg).abs().max())
    assert int(correct) == rh
    # rows of the gradient sum to S - S = 0
    assert float(grad.double().sum(1).abs().max()) <= C * 2.0 ** -23 / N


def test_target_given_as_nc11():
    x, t, t64 = _inputs(5, 10, True, torch.float32)
    L = SoftTargetCrossEntropyLoss(0.1)
    a = L.loss_and_grad(x, t)
    b = L.loss_and_grad(x, t.view(5, 10, 1, 1))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_oracle_methods_are_the_formulas():
    x, t, t64 = _inputs(5, 10, True, torch.float32)
    L = SoftTargetCrossEntropyLoss(0.1)
    rl, rg, _ = _formula(x, t64, 0.1)
    assert torch.allclose(L._cpu_loss(x, t).double(), rl, **TOL)
    assert torch.allclose(L._cpu_grad(x, t).double(), rg, **TOL)
    lab = torch.tensor([0, 3, 9, 3, 1])
    rl, rg, _ = _formula(x, torch.nn.functional.one_hot(lab, 10).double(), 0.1)
    assert torch.allclose(L._cpu_loss(x, lab).double(), rl, **TOL)
    assert torch.allclose(L._cpu_grad(x, lab).double(), rg, **TOL)


def test_half_half_target_old_kind_unchanged_new_kind_right():
    """A 0.5 / 0.5 target has no class above 0.5: softmax_crossentropy goes on reporting 0 (its rule
    is unchanged), soft_crossentropy reports the formula's value."""
    x = torch.tensor([[2.0, -1.0], [0.5, 0.25], [-3.0, 4.0]])
    t = torch.full((3, 2), 0.5)
    old = SoftmaxCrossEntropyLoss()
    lo, go, _ = old.loss_and_grad(x, t)
    assert float(lo) == 0.0 == float(old._cpu_loss(x, t))
    assert torch.allclose(go, old._cpu_grad(x, t), **TOL)
    rl, rg, _ = _formula(x, t.double(), 0.0)
    ln, gn, _ = LossFactory.create("soft_ce").loss_and_grad(x, t)
    assert float(rl) > 0.5
    assert torch.allclose(ln.double().reshape(()), rl, **TOL)
    assert torch.allclose(gn.double(), rg, **TOL)
    assert torch.allclose(gn, go, **TOL)  # the gradient was right all along
    # one class above 0.5 with weight 0.7: the old kind reports lse - x_hot, not the soft loss
    t7 = torch.tensor([[0.7, 0.3]] * 3)
    assert not torch.allclose(old.loss_and_grad(x, t7)[0], LossFactory.create("soft_ce").loss_and_grad(x, t7)[0],
                              **TOL)


@pytest.mark.parametrize("labels", [True, False])
def test_eps0_one_hot_agrees_with_softmax_crossentropy(labels):
    x, lab, t64 = _inputs(64, 200, False, torch.float32)
    tgt = lab if labels else t64.float()
    a = SoftmaxCrossEntropyLoss().loss_and_grad(x, tgt)
    b = SoftTargetCrossEntropyLoss(0.0).loss_and_grad(x, tgt)
    assert torch.allclose(a[0], b[0], **TOL) and torch.allclose(a[1], b[1], **TOL) and int(a[2]) == int(b[2])


def test_factory_aliases_and_config_round_trip():
    for name in ("soft_crossentropy", "soft_ce", "label_smoothing_ce"):
        L = LossFactory.create(name, label_smoothing=0.1)
        assert isinstance(L, SoftTargetCrossEntropyLoss) and L.kind == "soft_crossentropy"
        assert L.label_smoothing == pytest.approx(0.1)
    assert LossFactory.create("soft_crossentropy").label_smoothing == 0.0
    cfg = SoftTargetCrossEntropyLoss(0.2).get_config()
    assert cfg["type"] == "soft_crossentropy" and cfg["parameters"] == {"label_smoothing": 0.2}
    back = LossFactory.create_from_config(cfg)
    assert isinstance(back, SoftTargetCrossEntropyLoss) and back.label_smoothing == 0.2
    assert LossFactory.create_from_config(LossConfig("label_smoothing_ce", parameters={"label_smoothing": 0.3})
                                          ).label_smoothing == 0.3
    assert SoftTargetCrossEntropyLoss(0.25).clone().label_smoothing == 0.25
    assert LossFactory.create_soft_crossentropy(0.05).label_smoothing == 0.05


@pytest.mark.parametrize("eps", [-0.1, 1.0, 1.5, float("nan")])
def test_bad_label_smoothing_raises(eps):
    with pytest.raises(ValueError, match="label_smoothing"):
        SoftTargetCrossEntropyLoss(eps)
    with pytest.raises(ValueError, match="label_smoothing"):
        LossFactory.create("soft_crossentropy", label_smoothing=eps)


def test_native_kernel_checks_its_own_arguments():
    from dcnn_amd.ops import cpu
    x = torch.zeros(2, 3)
    with pytest.raises(ValueError, match="label_smoothing"):
        cpu.loss_fused(x, None, torch.tensor([0, 1]), "soft_crossentropy", 1.0)


def test_grad_scale_scales_the_gradient_not_the_loss():
    x, t, t64 = _inputs(5, 10, True, torch.float32)
    L = SoftTargetCrossEntropyLoss(0.1)
    l1, g1, _ = L.loss_and_grad(x, t)
    l2, g2, _ = L.loss_and_grad(x, t, grad_scale=0.25)
    assert torch.equal(l1, l2)
    assert torch.equal(g2, g1 * 0.25)
    _, rg, _ = _formula(x, t64, 0.1, 0.25)
    assert torch.allclose(g2.double(), rg, **TOL)
