"""Mixup / CutMix on the CPU: the per-batch draw ``mix_plan`` (csrc/native), the native ``mix_batch``
against a numpy float64 reference, ``BatchMixer`` and its place in the trainer."""
import math

import numpy as np
import pytest
import torch

from dcnn_amd.data import BatchMixer
from dcnn_amd.ops import cpu

STEPS = 20000


def _plans(seed, n, H, W, ma, ca, prob=1.0, sw=0.5):
    return [cpu.mix_plan(seed, s, H, W, ma, ca, prob, sw) for s in range(1, n + 1)]


# ------------------------------------------------------------------------------------------- plan
def test_plan_is_a_pure_function_of_seed_and_step():
    fwd = [cpu.mix_plan(3, s, 32, 32, 0.8, 1.0) for s in range(1, 200)]
    bwd = [cpu.mix_plan(3, s, 32, 32, 0.8, 1.0) for s in range(199, 0, -1)][::-1]
    assert fwd == bwd
    assert fwd != [cpu.mix_plan(4, s, 32, 32, 0.8, 1.0) for s in range(1, 200)]
    assert len(set(fwd)) > 150  # the steps differ from each other
    for mode, lam, yl, yh, xl, xh in fwd:
        assert mode in (1, 2) and 0.0 <= lam <= 1.0
        if mode == 1:
            assert (yl, yh, xl, xh) == (0, 0, 0, 0)


def test_prob_zero_never_mixes_and_single_alpha_fixes_the_mode():
    assert all(p == (0, 1.0, 0, 0, 0, 0) for p in _plans(0, 500, 16, 16, 0.8, 1.0, prob=0.0))
    assert all(p == (0, 1.0, 0, 0, 0, 0) for p in _plans(0, 500, 16, 16, 0.0, 0.0))
    assert all(p[0] == 1 for p in _plans(0, 500, 16, 16, 0.8, 0.0, sw=1.0))
    assert all(p[0] == 2 for p in _plans(0, 500, 16, 16, 0.0, 1.0, sw=0.0))
    assert all(p[0] == 2 for p in _plans(0, 500, 16, 16, 0.8, 1.0, sw=1.0))
    assert all(p[0] == 1 for p in _plans(0, 500, 16, 16, 0.8, 1.0, sw=0.0))


@pytest.mark.parametrize("prob,sw", [(0.7, 0.5), (0.3, 0.2), (1.0, 0.9)])
def test_mode_frequencies(prob, sw):
    modes = np.array([p[0] for p in _plans(5, STEPS, 8, 8, 0.8, 1.0, prob, sw)])
    f0 = float((modes == 0).mean())
    se0 = math.sqrt(prob * (1 - prob) / STEPS)
    assert abs(f0 - (1 - prob)) <= 5 * se0, (f0, 1 - prob, se0)
    mixed = modes[modes != 0]
    fc = float((mixed == 2).mean())
    sec = math.sqrt(sw * (1 - sw) / len(mixed))
    assert abs(fc - sw) <= 5 * sec, (fc, sw, sec)


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("alpha", [0.2, 0.8, 1.0])
def test_lambda_is_beta_distributed(alpha, seed):
    """Kolmogorov-Smirnov against Beta(alpha, alpha) below the 0.1 % critical value. The draws are
    fixed functions of the seed: a failure is a sampler bug."""
    from scipy import stats
    plans = _plans(seed, STEPS, 8, 8, alpha, 0.0)
    assert all(p[0] == 1 for p in plans)
    lam = np.array([p[1] for p in plans])
    d = stats.kstest(lam, stats.beta(alpha, alpha).cdf).statistic
    print(f"alpha {alpha} seed {seed}: KS {d:.5f} (bound {1.95 / math.sqrt(STEPS):.5f})")
    assert d < 1.95 / math.sqrt(STEPS)


@pytest.mark.parametrize("H,W", [(5, 5), (28, 28), (64, 48)])
def test_cutmix_boxes(H, W):
    plans = _plans(9, 5000, H, W, 0.0, 1.0)
    empty = top = bottom = 0
    for mode, lam, yl, yh, xl, xh in plans:
        assert mode == 2
        assert 0 <= yl <= yh <= H and 0 <= xl <= xh <= W
        area = (yh - yl) * (xh - xl)
        assert lam == (1.0 - area / (H * W) if area else 1.0)
        empty += area == 0
        top += area > 0 and yl == 0
        bottom += area > 0 and yh == H
    assert empty > 0  # lam near 1 gives an empty box (and lam = 1)
    assert top > 0 and bottom > 0  # boxes clipped at either edge occur
    assert len({p[2:] for p in plans}) > 20


@pytest.mark.parametrize("kw,word", [
    (dict(mixup_alpha=-0.5), "mixup_alpha -0.5"), (dict(cutmix_alpha=-1.0), "cutmix_alpha -1.0"),
    (dict(prob=1.5), "prob 1.5"), (dict(prob=-0.25), "prob -0.25"), (dict(switch_prob=2.0), "switch_prob 2.0"),
    (dict(H=0), "H 0"), (dict(W=-3), "W -3")])
def test_plan_bad_arguments(kw, word):
    a = dict(seed=0, step=1, H=8, W=8, mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5)
    a.update(kw)
    with pytest.raises(ValueError, match=word.replace(".", r"\.")):
        cpu.mix_plan(**a)


# ------------------------------------------------------------------------------------------ batch
ROWS = [(3, 5, 5), (1, 28, 28), (3, 32, 32)]
BATCHES = [1, 2, 5, 8]
KS = [3, 10, 200]


def boxes(H, W):
    """Full image, one pixel, touching each edge, empty."""
    return [(0, H, 0, W), (H // 2, H // 2 + 1, W // 2, W // 2 + 1), (0, 2, 1, W - 1), (H - 2, H, 1, W - 1),
            (1, H - 1, 0, 2), (1, H - 1, W - 2, W), (2, 2, 0, W)]


def ref_target(labels, K, mode, lam):
    B = len(labels)
    t = np.zeros((B, K), np.float32)
    lamf = np.float32(lam)
    for i in range(B):
        a, b = int(labels[i]), int(labels[B - 1 - i])
        if mode == 0 or a == b or B - 1 - i == i:
            if 0 <= a < K:
                t[i, a] = 1.0
        else:
            if 0 <= a < K:
                t[i, a] = lamf
            if 0 <= b < K:
                t[i, b] = np.float32(1.0) - lamf
    return t


def _data(B, row, K, dtype, seed=0):
    g = torch.Generator().manual_seed(seed + 17 * B + row[1])
    x = torch.randn((B,) + row, generator=g, dtype=torch.float64).to(dtype)
    lab = torch.randint(0, K, (B,), generator=g)
    if B >= 2:
        lab[-1] = lab[0]  # one pair with equal labels: exactly 1.0
    return x, lab


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("row", ROWS, ids=lambda r: "x".join(map(str, r)))
@pytest.mark.parametrize("B", BATCHES)
def test_mixup_against_float64(B, row, dtype):
    for K, lam in zip(KS, (0.3, 0.9172, 0.0)):
        x, lab = _data(B, row, K, dtype)
        x0 = x.clone()
        tgt = torch.full((B, K), -7.0)
        cpu.mix_batch(x, lab, tgt, 1, lam, (0, 0, 0, 0), K)
        a = x0.double().numpy()
        ref = lam * a + (1 - lam) * a[::-1]
        if B % 2:
            ref[B // 2] = a[B // 2]
            assert torch.equal(x[B // 2], x0[B // 2])  # the middle sample is not touched
        bound = 4 * 2.0 ** -24 * (np.abs(a) + np.abs(a[::-1]))
        err = np.abs(x.double().numpy() - ref)
        assert (err <= bound).all(), float((err - bound).max())
        assert np.array_equal(tgt.numpy(), ref_target(lab.numpy(), K, 1, lam))
        if B >= 2:
            assert float(tgt[0, lab[0]]) == 1.0
        if B == 1:
            assert torch.equal(x, x0)


@pytest.mark.parametrize("row", ROWS, ids=lambda r: "x".join(map(str, r)))
@pytest.mark.parametrize("B", BATCHES)
def test_cutmix_and_mode0_are_bit_exact(B, row):
    C, H, W = row
    for k, (yl, yh, xl, xh) in enumerate(boxes(H, W)):
        K = KS[k % 3]
        x, lab = _data(B, row, K, torch.float32, seed=k)
        x0 = x.clone()
        area = (yh - yl) * (xh - xl)
        lam = 1.0 - area / (H * W)
        tgt = torch.full((B, K), -7.0)
        cpu.mix_batch(x, lab, tgt, 2, lam, (yl, yh, xl, xh), K)
        ref = x0.clone()
        ref[:, :, yl:yh, xl:xh] = x0.flip(0)[:, :, yl:yh, xl:xh]
        assert torch.equal(x, ref)
        outside = torch.ones(H, W, dtype=torch.bool)
        outside[yl:yh, xl:xh] = False
        assert torch.equal(x[:, :, outside], x0[:, :, outside])
        assert np.array_equal(tgt.numpy(), ref_target(lab.numpy(), K, 2, lam))
    x, lab = _data(B, row, 10, torch.float32)
    x0 = x.clone()
    tgt = torch.full((B, 10), -7.0)
    cpu.mix_batch(x, lab, tgt, 0, 0.25, (0, 0, 0, 0), 10)
    assert torch.equal(x, x0)
    assert torch.equal(tgt, torch.nn.functional.one_hot(lab, 10).float())


def test_labels_outside_the_classes_contribute_nothing():
    x = torch.randn(4, 1, 4, 4)
    lab = torch.tensor([-1, 2, 7, 3])
    tgt = torch.full((4, 5), -7.0)
    cpu.mix_batch(x, lab, tgt, 1, 0.25, (0, 0, 0, 0), 5)
    assert np.array_equal(tgt.numpy(), ref_target(lab.numpy(), 5, 1, 0.25))
    assert tgt[2].abs().sum() == 0.75 and tgt[0].abs().sum() == 0.75 and tgt[1].sum() == 0.25


@pytest.mark.parametrize("kw,word", [
    (dict(lam=1.5), "lam 1.5"), (dict(lam=-0.1), "lam -0.1"), (dict(K=0), "num_classes 0"), (dict(mode=3), "mode 3"),
    (dict(mode=2, box=(0, 9, 0, 4)), r"\[0, 9\)"), (dict(mode=2, box=(3, 2, 0, 4)), r"\[3, 2\)"),
    (dict(mode=2, box=(0, 4, -1, 4)), r"\[-1, 4\)"), (dict(mode=2, box=(0, 4, 0, 9)), r"\[0, 9\)")])
def test_mix_batch_bad_arguments(kw, word):
    a = dict(mode=1, lam=0.5, box=(0, 0, 0, 0), K=5)
    a.update(kw)
    x = torch.zeros(2, 1, 8, 8)
    tgt = torch.zeros(2, max(a["K"], 1))
    with pytest.raises(ValueError, match=word):
        cpu.mix_batch(x, torch.zeros(2, dtype=torch.int64), tgt, a["mode"], a["lam"], a["box"], a["K"])


def test_more_than_int32_elements_raises():
    with pytest.raises(ValueError, match="exceed 2\\^31 - 1"):
        cpu.C().mix_check(1 << 16, 1 << 8, 1 << 4, 1 << 4, 10, 1, 0.5, 0, 0, 0, 0)


# ------------------------------------------------------------------------------------------ mixer
def test_batch_mixer_follows_its_plan_and_resumes():
    m = BatchMixer(10, seed=4)
    x0 = torch.randn(6, 3, 8, 8, generator=torch.Generator().manual_seed(0))
    lab = torch.tensor([0, 1, 2, 3, 4, 5])
    outs = []
    for step in range(1, 6):
        x, t = m(x0.clone(), lab)
        assert m.state == step and t.shape == (6, 10) and t.dtype == torch.float32
        mode, lam, yl, yh, xl, xh = m.plan(step)
        assert m.state == step  # plan() has no side effects
        xr, tr = x0.clone(), torch.empty(6, 10)
        cpu.mix_batch(xr, lab, tr, mode, lam, (yl, yh, xl, xh), 10)
        assert torch.equal(x, xr) and torch.equal(t, tr)
        assert torch.allclose(t.sum(1), torch.ones(6), atol=1e-6)
        outs.append((x, t))
    r = BatchMixer(10, seed=4)
    r.state = 3
    x, t = r(x0.clone(), lab)
    assert torch.equal(x, outs[3][0]) and torch.equal(t, outs[3][1])
    none = BatchMixer(10, mixup_alpha=0.0, cutmix_alpha=0.0)
    x, t = none(x0.clone(), lab)  # dense targets for an unmixed batch too
    assert torch.equal(x, x0) and torch.equal(t, torch.nn.functional.one_hot(lab, 10).float())
    with pytest.raises(ValueError):
        BatchMixer(0)
    with pytest.raises(ValueError):
        BatchMixer(10, mixup_alpha=-1.0)
    with pytest.raises(ValueError):
        BatchMixer(10, prob=1.5)


def _small_cnn():
    from dcnn_amd.nn import SequentialBuilder
    m = (SequentialBuilder("mix_cnn").input([3, 8, 8]).conv2d(4, 3, 3, 1, 1, 1, 1, True, "c1").activation("relu", "r1")
         .flatten("f").dense(5, True, "fc").build())
    m.set_seed(3)
    m.initialize()
    return m


class _SpyMixer(BatchMixer):
    def __call__(self, x, labels):
        x, t = super().__call__(x, labels)
        self.targets = getattr(self, "targets", []) + [t.clone()]
        return x, t


def _loader():
    from dcnn_amd.data import ArrayDataLoader
    g = np.random.default_rng(0)
    ld = ArrayDataLoader(g.standard_normal((24, 3, 8, 8)).astype(np.float32), g.integers(0, 5, 24), batch_size=8)
    ld.num_classes = 5
    return ld


def test_trainer_with_a_mixer(tmp_path):
    from dcnn_amd.nn import Adam, LossFactory, TrainingConfig, load_checkpoint, save_checkpoint, train_class_epoch
    m, ld = _small_cnn(), _loader()
    opt = Adam(1e-3)
    opt.attach(m)
    mixer = _SpyMixer(5, seed=1)
    cfg = TrainingConfig(batch_size=8, progress_print_interval=0)
    loss, acc = train_class_epoch(m, ld, opt, LossFactory.create("soft_crossentropy", label_smoothing=0.1), cfg,
                                  mixer=mixer)
    assert math.isfinite(loss) and loss > 0 and 0.0 <= acc <= 1.0
    assert mixer.state == 3 and len(mixer.targets) == 3
    for t in mixer.targets:
        assert t.shape == (8, 5) and float((t.sum(1) - 1).abs().max()) <= 1e-6
    with pytest.raises(ValueError, match="silently wrong"):
        train_class_epoch(m, ld, opt, LossFactory.create("softmax_crossentropy"), cfg, mixer=mixer)
    # the counter travels in the .state sidecar
    save_checkpoint(m, opt, str(tmp_path / "ck"), 1, mixer=mixer)
    fresh = BatchMixer(5, seed=1)
    load_checkpoint(m, opt, str(tmp_path / "ck"), mixer=fresh)
    assert fresh.state == 3


def test_training_config_defaults_build_no_mixer(monkeypatch):
    from dcnn_amd.nn import TrainingConfig
    from dcnn_amd.nn.train import build_mixer
    cfg = TrainingConfig()
    assert (cfg.mixup_alpha, cfg.cutmix_alpha, cfg.mix_prob, cfg.mix_switch_prob, cfg.label_smoothing) == \
        (0.0, 0.0, 1.0, 0.5, 0.0)
    assert build_mixer(cfg, 10) is None
    for k in ("MIXUP_ALPHA", "CUTMIX_ALPHA", "MIX_PROB", "MIX_SWITCH_PROB", "LABEL_SMOOTHING"):
        monkeypatch.delenv(k, raising=False)
    assert build_mixer(TrainingConfig().load_from_env(), 10) is None
    monkeypatch.setenv("MIXUP_ALPHA", "0.8")
    monkeypatch.setenv("CUTMIX_ALPHA", "1.0")
    monkeypatch.setenv("MIX_PROB", "0.9")
    monkeypatch.setenv("MIX_SWITCH_PROB", "0.25")
    monkeypatch.setenv("LABEL_SMOOTHING", "0.1")
    cfg = TrainingConfig().load_from_env()
    assert (cfg.mixup_alpha, cfg.cutmix_alpha, cfg.mix_prob, cfg.mix_switch_prob, cfg.label_smoothing) == \
        (0.8, 1.0, 0.9, 0.25, 0.1)
    mx = build_mixer(cfg, 10, seed=2)
    assert isinstance(mx, BatchMixer) and mx.get_config() == dict(num_classes=10, mixup_alpha=0.8, cutmix_alpha=1.0,
                                                                  prob=0.9, switch_prob=0.25, seed=2)
