"""Mixup / CutMix on the GPU (csrc/kernels/mix.hip): the kernel against the native CPU backend bit for
bit (that one is checked against a float64 reference in tests/test_batch_mix_cpu.py), the mixer
inside the HBM-resident loader, and a captured training step on mixed batches."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = [(3, 5, 5), (1, 28, 28), (3, 32, 32)]  # 75 floats (no multiple of 4), 784, 3072 (two chunks)
BATCHES = [1, 2, 5, 8]
KS = [3, 10, 200, 1000]


def boxes(H, W):
    """Full image, one pixel, touching each edge, empty."""
    return [(0, H, 0, W), (H // 2, H // 2 + 1, W // 2, W // 2 + 1), (0, 2, 1, W - 1), (H - 2, H, 1, W - 1),
            (1, H - 1, 0, 2), (1, H - 1, W - 2, W), (2, 2, 0, W)]


def _data(B, row, K, seed=0):
    g = torch.Generator().manual_seed(seed + 17 * B + row[1])
    x = torch.randn((B,) + row, generator=g)
    lab = torch.randint(0, K, (B,), generator=g)
    if B >= 2:
        lab[-1] = lab[0]  # one pair with equal labels: exactly 1.0
    if B >= 5:
        lab[1] = K + 3  # a label outside [0, K) contributes nothing
    return x, lab


def _both(x, lab, K, mode, lam, box):
    from dcnn_amd.ops import cpu, hip
    xc, tc = x.clone(), torch.full((x.shape[0], K), -7.0)
    cpu.mix_batch(xc, lab, tc, mode, lam, box, K)
    xg, tg = x.cuda(), torch.full((x.shape[0], K), -7.0, device="cuda")
    hip.mix_batch(xg, lab.cuda(), tg, mode, lam, box, K)
    torch.cuda.synchronize()
    return xc, tc, xg.cpu(), tg.cpu()


@pytest.mark.parametrize("row", ROWS, ids=lambda r: "x".join(map(str, r)))
@pytest.mark.parametrize("B", BATCHES)
def test_gpu_equals_cpu_bit_for_bit(B, row):
    C, H, W = row
    cases = [(0, 0.4, (0, 0, 0, 0))] + [(1, lam, (0, 0, 0, 0)) for lam in (0.3, 0.9172, 0.0, 1.0)]
    cases += [(2, 1.0 - (b[1] - b[0]) * (b[3] - b[2]) / (H * W), b) for b in boxes(H, W)]
    for k, (mode, lam, box) in enumerate(cases):
        K = KS[k % len(KS)]
        x, lab = _data(B, row, K, seed=k)
        xc, tc, xg, tg = _both(x, lab, K, mode, lam, box)
        assert torch.equal(xg, xc), (mode, lam, box)
        assert torch.equal(tg, tc), (mode, lam, box, K)
        if mode == 0 or B == 1:
            assert torch.equal(xg, x)
        if mode == 1 and B % 2:
            assert torch.equal(xg[B // 2], x[B // 2])
        if B >= 2:
            assert float(tg[0, lab[0]]) == 1.0


def test_misaligned_views_take_the_unaligned_path():
    """A batch that starts 4 bytes into an allocation and a target with K % 4 != 0."""
    from dcnn_amd.ops import cpu, hip
    B, row, K = 6, (3, 8, 8), 10
    x, lab = _data(B, row, K)
    buf = torch.zeros(x.numel() + 1, device="cuda")
    xg = buf[1:].view(x.shape)
    xg.copy_(x)
    tg = torch.full((B, K), -7.0, device="cuda")
    hip.mix_batch(xg, lab.cuda(), tg, 1, 0.37, (0, 0, 0, 0), K)
    xc, tc = x.clone(), torch.empty(B, K)
    cpu.mix_batch(xc, lab, tc, 1, 0.37, (0, 0, 0, 0), K)
    assert torch.equal(xg.cpu(), xc) and torch.equal(tg.cpu(), tc) and float(buf[0]) == 0.0


@pytest.mark.parametrize("kw,word", [
    (dict(lam=1.5), "lam 1.5"), (dict(K=0), "num_classes 0"), (dict(mode=3), "mode 3"),
    (dict(mode=2, box=(0, 9, 0, 4)), r"\[0, 9\)"), (dict(mode=2, box=(0, 4, -1, 4)), r"\[-1, 4\)")])
def test_bad_arguments_raise_before_any_launch(kw, word):
    from dcnn_amd.ops import hip
    a = dict(mode=1, lam=0.5, box=(0, 0, 0, 0), K=5)
    a.update(kw)
    x = torch.zeros(2, 1, 8, 8, device="cuda")
    tgt = torch.zeros(2, max(a["K"], 1), device="cuda")
    with pytest.raises(ValueError, match=word):
        hip.mix_batch(x, torch.zeros(2, dtype=torch.int64, device="cuda"), tgt, a["mode"], a["lam"], a["box"], a["K"])


def _loaders(n=40, K=7, batch=8):
    from dcnn_amd.data import AugmentationBuilder, DeviceDataLoader
    g = np.random.default_rng(3)
    data = (g.integers(0, 256, (n, 3, 16, 16)) / np.float32(255)).astype(np.float32)
    labels = g.integers(0, K, n)
    out = []
    for _ in range(2):
        ld = DeviceDataLoader(data=data, labels=labels, num_classes=K, batch_size=batch, shuffle=True, seed=5)
        ld.set_augmentation(AugmentationBuilder().horizontal_flip(0.5).random_crop(1.0, 2).build())
        ld.reset()
        out.append(ld)
    return out


def test_loader_with_a_mixer():
    from dcnn_amd.data import BatchMixer
    from dcnn_amd.ops import cpu
    K = 7
    plain, mixed = _loaders(K=K)
    mixer = BatchMixer(K, seed=2)
    mixed.set_mixer(mixer)
    modes = set()
    for step in range(1, 6):
        x0, y0 = plain.get_next_batch()
        x, t = mixed.get_next_batch()
        assert t.shape == (8, K) and t.dtype == torch.float32 and t.is_cuda and mixer.state == step
        mode, lam, yl, yh, xl, xh = mixer.plan(step)
        modes.add(mode)
        xr, tr = x0.cpu().clone(), torch.empty(8, K)
        cpu.mix_batch(xr, y0.cpu(), tr, mode, lam, (yl, yh, xl, xh), K)
        assert torch.equal(x.cpu(), xr) and torch.equal(t.cpu(), tr)
    assert modes == {1, 2}
    # dense targets for a batch that is not mixed, too
    plain, mixed = _loaders(K=K)
    mixed.set_mixer(BatchMixer(K, prob=0.0))
    x0, y0 = plain.get_next_batch()
    x, t = mixed.get_next_batch()
    assert torch.equal(x, x0) and torch.equal(t, torch.nn.functional.one_hot(y0, K).float())


def _tiny(seed=1):
    from dcnn_amd.nn import Adam, LossFactory, SequentialBuilder
    m = (SequentialBuilder("mix_step").input([3, 16, 16]).conv2d(8, 3, 3, 1, 1, 1, 1, False, "conv")
         .batchnorm(1e-5, 0.1, True, "bn").activation("relu", "relu").avgpool2d(16, 16, 1, 1, 0, 0, "pool")
         .flatten("flatten").dense(10, True, "fc").build())
    m.set_seed(seed)
    m.set_device("GPU:0")
    m.initialize()
    opt = Adam(1e-2)
    opt.attach(m)
    return m, opt, LossFactory.create("soft_crossentropy", label_smoothing=0.1)


def test_captured_step_on_mixed_batches_equals_eager():
    from dcnn_amd.data import BatchMixer
    from dcnn_amd.runtime.step import TrainStep
    g = torch.Generator().manual_seed(0)
    xs = [torch.randn(8, 3, 16, 16, generator=g).cuda() for _ in range(3)]
    ys = [torch.randint(0, 10, (8,), generator=g).cuda() for _ in range(3)]
    me, oe, le = _tiny()
    mg, og, lg = _tiny()
    se, sg = TrainStep(me, le, oe, use_graph=False), TrainStep(mg, lg, og, use_graph=True)
    mxe, mxg = BatchMixer(10, seed=6), BatchMixer(10, seed=6)
    for k in range(3):
        xe, te = mxe(xs[k].clone(), ys[k])
        xg, tg = mxg(xs[k].clone(), ys[k])
        assert torch.equal(xe, xg) and torch.equal(te, tg) and te.shape == (8, 10)
        se(xe, te)
        sg(xg, tg)
        torch.cuda.synchronize()
        assert float(sg.last_loss.item()) == float(se.last_loss.item()) and np.isfinite(float(se.last_loss.item()))
        assert torch.equal(mg.arena.data, me.arena.data)
    assert sg.graphs is not None
