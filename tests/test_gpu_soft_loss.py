"""Soft-target cross entropy with label smoothing on the GPU (csrc/kernels/loss_optim.hip, loss kind 6)
against the native CPU backend (tests/test_soft_loss_cpu.py checks that one against the formulas).

Shapes: N = 4 is the single-workgroup path, 5 the first ticketed one, 257 makes the last workgroup
loop over its rows; C = 3 / 64 / 65 / 200 / 1000 put lane tails on both sides of a wave. Bounds: fp32
logits as tests/test_gpu_kernels.py::test_loss_fused (the same kernel and its __expf); bf16 logits
against the CPU on the same bf16-rounded logits, gradient at the project's bf16 bound 1e-2."""
import pytest
import torch

pytestmark = pytest.mark.gpu

NS = [1, 4, 5, 64, 257]
CS = [3, 64, 65, 200, 1000]
BF16 = torch.bfloat16


def rel_err(a, b):
    a = a.double().cpu()
    b = b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _case(N, C, bf16):
    g = torch.Generator().manual_seed(100 * N + C)
    x = 3.0 * torch.randn(N, C, generator=g)
    if bf16:
        x = x.to(BF16).float()
    # a clear winner per row (0.5 above the rest: far more than the bf16 step 2^-5 at this magnitude)
    win = torch.randint(0, C, (N,), generator=g)
    x[torch.arange(N), win] = (x.max(1).values + 0.5).to(BF16).float()
    lab = torch.randint(0, C, (N,), generator=g)
    lab[::2] = win[::2]  # half of the rows are hits
    lam = torch.rand(N, generator=g) * 0.4 + 0.55  # labels[n] keeps the larger share
    other = torch.randint(0, C, (N,), generator=g)
    t = torch.zeros(N, C)
    t[torch.arange(N), lab] += lam
    t[torch.arange(N), other] += 1 - lam
    return x, lab, t


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("N", NS)
def test_gpu_matches_the_cpu_backend(N, C, bf16):
    from dcnn_amd.nn import SoftTargetCrossEntropyLoss
    x, lab, t = _case(N, C, bf16)
    xg = x.cuda().to(BF16) if bf16 else x.cuda()
    for eps in (0.0, 0.1):
        L = SoftTargetCrossEntropyLoss(eps)
        for tgt in (t, lab):
            lc, gc, cc = L.loss_and_grad(x, tgt)
            lg, gg, cg = L.loss_and_grad(xg, tgt.cuda())
            torch.cuda.synchronize()
            dl, dg = abs(lg.item() - lc.item()), rel_err(gg, gc)
            print(f"N {N} C {C} eps {eps} {'dense' if tgt.dim() == 2 else 'labels'}: |dloss| {dl:.3e} grad {dg:.3e}")
            assert gg.dtype == xg.dtype and gg.shape == xg.shape
            assert dl < 1e-4 * max(1, abs(lc.item()))
            assert dg < (1e-2 if bf16 else 1e-4)
            assert cg.item() == cc.item()
            assert 0 < cc.item() or N == 1
        # the [N, C, 1, 1] form of the target
        lg4, gg4, _ = L.loss_and_grad(xg, t.view(N, C, 1, 1).cuda())
        lg2, gg2, _ = L.loss_and_grad(xg, t.cuda())
        assert torch.equal(lg4, lg2) and torch.equal(gg4, gg2)


@pytest.mark.parametrize("N", [4, 5, 257])
def test_bit_reproducible_and_grad_scale(N):
    from dcnn_amd.nn import SoftTargetCrossEntropyLoss
    x, lab, t = _case(N, 200, False)
    xg, tg = x.cuda(), t.cuda()
    L = SoftTargetCrossEntropyLoss(0.1)
    a = L.loss_and_grad(xg, tg)
    b = L.loss_and_grad(xg, tg)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    s = L.loss_and_grad(xg, tg, grad_scale=0.25)
    assert torch.equal(s[0], a[0]) and torch.equal(s[2], a[2])
    assert torch.equal(s[1], a[1] * 0.25)  # a power of two: exact


@pytest.mark.parametrize("N", [4, 64])
def test_graph_replays_give_the_eager_bits(N):
    """Captured as runtime/step.py does (side-stream warm-up, torch.cuda.graph on that stream) and
    replayed three times: every replay gives the eager bits, so the ticket resets itself."""
    from dcnn_amd.nn import SoftTargetCrossEntropyLoss
    from dcnn_amd.runtime.capture import capture_guard
    x, lab, t = _case(N, 200, False)
    xg, tg = x.cuda(), t.cuda()
    L = SoftTargetCrossEntropyLoss(0.1)
    el, eg, ec = L.loss_and_grad(xg, tg)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            L.loss_and_grad(xg, tg)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with capture_guard(), torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
        gl, gg, gc = L.loss_and_grad(xg, tg)
    for _ in range(3):
        gl.fill_(-1.0)
        gg.zero_()
        gc.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(gl, el) and torch.equal(gg, eg) and torch.equal(gc, ec)


def test_bad_label_smoothing_raises_in_the_launcher():
    from dcnn_amd.ops import hip
    x = torch.zeros(2, 3, device="cuda")
    with pytest.raises(ValueError, match="label_smoothing"):
        hip.loss_fused(x, None, torch.zeros(2, dtype=torch.int64, device="cuda"), "soft_crossentropy", 1.0)
