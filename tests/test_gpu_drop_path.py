"""DropPath on the GPU at the kernel level (droppath.hip and the drop tail of lnorm.hip): the mask
against the CPU function bit for bit, the standalone per-sample scale, the fused LayerScale tail
x + m[n] gamma F(x) with its backward against a float64 reference (the metrics and bounds of
tests/test_gpu_lnorm.py::test_lscale), and a captured forward + backward replayed with a new mask
every time."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CL = torch.channels_last
BF16 = torch.bfloat16
F32 = torch.float32


def rel_err(a, b):
    a = a.double().cpu()
    b = b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def elem_excess(y, ref, abs_term=1e-5):
    """max over elements of |y - ref| / (2^-7 |ref| + abs_term): <= 1 passes."""
    y = y.double().cpu()
    return ((y - ref).abs() / (ref.abs() * 2.0 ** -7 + abs_term)).max().item()


@pytest.fixture(scope="module")
def hip():
    from dcnn_amd.ops import hip as h
    from dcnn_amd.ops._ext import kernels
    assert kernels().arch == "gfx950"
    return h


def cpu_mask(seed, draw, n, p):
    from dcnn_amd.ops import cpu
    return cpu.drop_path_mask(seed, draw, n, p)


def dev(t, dtype):
    t = t.to(dtype).cuda()
    return t.contiguous(memory_format=CL) if t.dim() == 4 else t.contiguous()


# ---------------------------------------------------------------------------------------- mask
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("seed", [1, (1 << 40) + 3])
def test_mask_equals_cpu(hip, seed, p):
    from dcnn_amd.ops._ext import kernels
    for draw in (1, 2, 1000):
        for n in (1, 3, 4, 5, 257):
            ref = cpu_mask(seed, draw, n, p)
            got = torch.tensor(kernels().drop_path_mask(seed, draw, n, p), dtype=F32)
            assert torch.equal(got, ref), (seed, draw, n, p)
            buf = torch.full((n,), -1.0, device="cuda")
            hip.drop_path_mask(buf, p, seed, draw=draw)
            assert torch.equal(buf.cpu(), ref)
            slot = torch.tensor([draw], dtype=torch.int64, device="cuda")  # the draw index read on the device
            hip.drop_path_mask(buf.fill_(-1.0), p, seed, slot=slot)
            assert torch.equal(buf.cpu(), ref)


def test_mask_rate_out_of_range(hip):
    from dcnn_amd.ops._ext import kernels
    for p in (-0.5, 1.0):
        with pytest.raises(Exception, match="rate"):
            kernels().drop_path_mask(1, 1, 4, p)


# ------------------------------------------------------------------------- standalone scale
SCALE_CASES = [((5, 8, 3, 3), BF16), ((3, 96, 7, 5), BF16), ((2, 2048, 1, 1), BF16), ((4, 4, 2, 2), F32),
               ((3, 7), F32)]


def _layer(p, seed, dtype):
    from dcnn_amd.nn.layers import DropPath
    l = DropPath(p, "dp", seed)
    l.set_device("GPU:0")
    l.set_compute_dtype(dtype)
    return l


def _check_scale(l, x, dy, draw, seed, p):
    y = l.forward(x)
    m = l.last_mask()
    assert m.is_cuda and torch.equal(m.cpu(), cpu_mask(seed, draw, x.shape[0], p))
    dx = l.backward(dy)
    torch.cuda.synchronize()
    mv = m.view(-1, *([1] * (x.dim() - 1)))
    assert y.dtype == x.dtype and tuple(y.shape) == tuple(x.shape)
    assert torch.equal(y, (x.float() * mv).to(x.dtype))
    assert torch.equal(dx, (dy.float() * mv).to(x.dtype))
    for n in range(x.shape[0]):
        if m[n] == 0:
            assert (y[n] == 0).all() and (dx[n] == 0).all()
    return m.cpu()


@pytest.mark.parametrize("shape,dtype", SCALE_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)[6:])
def test_standalone_scale(hip, shape, dtype):
    g = torch.Generator().manual_seed(sum(shape))
    seed = 5
    ms = []
    l = _layer(0.5, seed, dtype)
    for draw in (1, 2, 3):  # three draws: with N >= 2 both outcomes turn up among them
        x, dy = dev(torch.randn(shape, generator=g), dtype), dev(torch.randn(shape, generator=g), dtype)
        ms.append(_check_scale(l, x, dy, draw, seed, 0.5))
    allm = torch.cat(ms)
    assert (allm == 0).any() and (allm != 0).any()


def test_standalone_scale_single_sample_both_outcomes(hip):
    shape, seed = (1, 16, 2, 2), 3
    l = _layer(0.5, seed, BF16)
    g = torch.Generator().manual_seed(2)
    ms = []
    for draw in range(1, 9):
        x, dy = dev(torch.randn(shape, generator=g), BF16), dev(torch.randn(shape, generator=g), BF16)
        ms.append(_check_scale(l, x, dy, draw, seed, 0.5))
    allm = torch.cat(ms)
    assert (allm == 0).any() and (allm != 0).any()


def test_standalone_scale_with_residual_and_nan_input(hip):
    """(+ residual) in the same store; a dropped sample's x is never read, so a NaN there does not leak."""
    x = torch.randn(4, 6, 5, generator=torch.Generator().manual_seed(1))
    res = torch.randn(4, 6, 5, generator=torch.Generator().manual_seed(2))
    mask = torch.tensor([2.0, 0.0, 2.0, 0.0])
    x[1] = float("nan")
    y = hip.drop_path_scale(x.cuda(), mask.cuda(), res.cuda())
    ref = torch.where(mask.view(-1, 1, 1) != 0, x * mask.view(-1, 1, 1), torch.zeros(())) + res
    assert torch.allclose(y.cpu(), ref, rtol=1e-6, atol=1e-6) and torch.equal(y[1].cpu(), res[1])
    # a dense view that does not start on a 16-byte boundary is a legitimate input (batch[k:] of odd rows)
    base = torch.randn(4 * 13 + 3, device="cuda")
    xv = base[3:].view(4, 13)
    assert xv.data_ptr() % 16 != 0
    assert torch.equal(hip.drop_path_scale(xv, mask.cuda()), xv * mask.cuda().view(-1, 1))
    batch = torch.randn(7, 7, device="cuda")  # rows of 7 floats: batch[3:] starts at byte 84
    l = _layer(0.5, 5, F32)
    xs = batch[3:]
    assert xs.data_ptr() % 16 != 0
    ys = l.forward(xs)
    ms = l.last_mask()
    assert torch.equal(ys, xs * ms.view(-1, 1)) and torch.equal(l.backward(xs), xs * ms.view(-1, 1))
    with pytest.raises(Exception, match="modulo 16"):  # the launcher itself still refuses a mismatch
        from dcnn_amd.ops._ext import kernels, stream_ptr
        out = torch.empty(4, 13, device="cuda")
        kernels().drop_path_scale(0, xv.data_ptr(), mask.cuda().data_ptr(), 0, out.data_ptr(), 4, 13, stream_ptr())
    xb = dev(torch.randn(4, 13), BF16)
    yb = hip.drop_path_scale(xb, mask.cuda())
    assert torch.equal(yb, (xb.float() * mask.cuda().view(-1, 1)).to(BF16))


# ------------------------------------------------------------------------------- fused tail
TAIL_CASES = [(6, 16, 4, 4), (5, 96, 3, 3), (2, 2048, 1, 1)]
_REF = {}


def tail_reference(case, dtype):
    """Operands (rounded to bf16 for the bf16 run), a mask with both kinds of sample, and the float64
    results; once per (case, dtype)."""
    key = (case, dtype)
    if key in _REF:
        return _REF[key]
    N, C = case[0], case[1]
    g = torch.Generator().manual_seed(977)
    rnd = (lambda t: t.to(BF16).float()) if dtype == BF16 else (lambda t: t)
    x, dy, res = (rnd(torch.randn(case, generator=g)) for _ in range(3))
    gamma = 1.0 + 0.5 * torch.randn(C, generator=g)
    seed = next(s for s in range(1, 64) if 0 < int((cpu_mask(s, 1, N, 0.5) != 0).sum()) < N)
    mask = cpu_mask(seed, 1, N, 0.5)
    assert (mask == 0).any() and (mask != 0).any()
    md, gd = mask.double().view(-1, 1, 1, 1), gamma.double().view(1, -1, 1, 1)
    r = dict(x=x, dy=dy, res=res, gamma=gamma, mask=mask, seed=seed,
             y=res.double() + md * gd * x.double(), dx=md * gd * dy.double(),
             dgamma=(md * dy.double() * x.double()).sum((0, 2, 3)))
    _REF[key] = r
    return r


def run_tail(hip, r, dtype, mask=None):
    x, dy, res = dev(r["x"], dtype), dev(r["dy"], dtype), dev(r["res"], dtype)
    gamma = r["gamma"].cuda()
    m = (r["mask"] if mask is None else mask).cuda()
    y = hip.lscale_drop_fwd(x, gamma, m, res)
    dg = torch.ones(gamma.numel(), device="cuda")
    dx = hip.lscale_drop_bwd(dy, x, gamma, m, dg)
    torch.cuda.synchronize()
    assert y.dtype == dtype and dx.dtype == dtype and y.is_contiguous(memory_format=CL)
    return y, dx, dg, res


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("case", TAIL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_fused_tail(hip, case, dtype):
    r = tail_reference(case, dtype)
    y, dx, dg, res = run_tail(hip, r, dtype)
    ey, ex, eg = rel_err(y, r["y"]), rel_err(dx, r["dx"]), rel_err(dg, r["dgamma"] + 1)
    print(f"y {ey:.3e} dx {ex:.3e} dgamma {eg:.2e}")
    if dtype == F32:
        assert ey < 1e-4 and ex < 1e-4 and eg < 1e-4
    else:
        xy, xx = elem_excess(y, r["y"]), elem_excess(dx, r["dx"])
        print(f"elem y {xy:.3f} dx {xx:.3f}")
        assert ey < 1e-2 and xy <= 1.0
        assert ex < 1e-2 and xx <= 1.0
        assert eg < 1e-4
    for n in range(case[0]):
        if r["mask"][n] == 0:  # the residual rows copied, the gradient exactly zero
            assert torch.equal(y[n], res[n]) and (dx[n] == 0).all()
    y2, dx2, dg2, _ = run_tail(hip, r, dtype)
    assert torch.equal(dg, dg2) and torch.equal(y, y2) and torch.equal(dx, dx2)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("case", TAIL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_fused_tail_with_unit_mask_is_the_scale_tail(hip, case, dtype):
    """mask = 1.0 everywhere: bit-identical to lscale_fwd (+ residual) / lscale_bwd."""
    r = tail_reference(case, dtype)
    y, dx, dg, res = run_tail(hip, r, dtype, mask=torch.ones(case[0]))
    x, dy, gamma = dev(r["x"], dtype), dev(r["dy"], dtype), r["gamma"].cuda()
    y0 = hip.lscale_fwd(x, gamma, res)
    dg0 = torch.ones(gamma.numel(), device="cuda")
    dx0 = hip.lscale_bwd(dy, x, gamma, dg0)
    torch.cuda.synchronize()
    assert torch.equal(y, y0) and torch.equal(dx, dx0) and torch.equal(dg, dg0)


def test_fused_tail_dropped_sample_is_not_read(hip):
    r = dict(tail_reference(TAIL_CASES[0], F32))
    x = r["x"].clone()
    x[r["mask"] == 0] = float("nan")
    r["x"] = x
    y, dx, dg, res = run_tail(hip, r, F32)
    assert torch.isfinite(y).all() and torch.isfinite(dx).all() and torch.isfinite(dg).all()


def test_fused_tail_unsupported_shapes(hip):
    m = torch.ones(4, device="cuda")
    for C, dtype in ((12, BF16), (4096, BF16), (4096, F32)):
        x = torch.zeros(4, C, 1, 1, device="cuda", dtype=dtype).contiguous(memory_format=CL)
        g = torch.ones(C, device="cuda")
        with pytest.raises(ValueError, match=str(C)):
            hip.lscale_drop_fwd(x, g, m, x)
        with pytest.raises(ValueError, match=str(C)):
            hip.lscale_drop_bwd(x, x, g, m, torch.zeros(C, device="cuda"))


# ----------------------------------------------------------------------------------- replay
def _replay_model(seed):
    """A model whose only layers are a DropPath and the dense layer the optimizer needs: the step's
    mask is readable after every replay, and y / dx follow from the loss and the weights."""
    from dcnn_amd.nn import SGD, LossFactory, SequentialBuilder
    m = (SequentialBuilder("dp_replay").input([32, 1, 1]).drop_path(0.5, "dp", seed=seed).flatten("flatten")
         .dense(10, True, "fc").build())
    m.set_seed(1)
    m.set_device("GPU:0")
    m.initialize()
    opt = SGD(0.05)
    opt.attach(m)
    return m, opt, LossFactory.create("softmax_crossentropy")


def test_replay_draws_a_new_mask_every_time(hip):
    """A step captured as runtime/step.py captures it, replayed 3 times at N = 64, p = 0.5."""
    from dcnn_amd.runtime.step import TrainStep
    seed, N = 31, 64
    torch.manual_seed(0)
    xs = [torch.randn(N, 32, 1, 1, device="cuda") for _ in range(3)]
    ys = [torch.randint(0, 10, (N,), device="cuda") for _ in range(3)]
    me, oe, le = _replay_model(seed)
    mg, og, lg = _replay_model(seed)
    se, sg = TrainStep(me, le, oe, use_graph=False), TrainStep(mg, lg, og, use_graph=True)
    masks = []
    for k in range(3):
        se(xs[k], ys[k])
        sg(xs[k], ys[k])
        torch.cuda.synchronize()
        mk = mg.layers[0].last_mask().cpu()
        masks.append(mk)
        # replay k == the eager run at draw index k + 1 with the same seed, bit for bit
        assert torch.equal(mk, cpu_mask(seed, k + 1, N, 0.5))
        assert torch.equal(mk, me.layers[0].last_mask().cpu())
        assert float(sg.last_loss.item()) == float(se.last_loss.item())
        assert torch.equal(mg.arena.data, me.arena.data)
    assert sg.graphs is not None
    for i in range(3):
        for j in range(i + 1, 3):
            assert not torch.equal(masks[i], masks[j])


def test_captured_forward_backward_matches_its_own_mask(hip):
    """The layer's forward + backward captured in a graph (as runtime/step.py does: a side-stream
    warm-up, then torch.cuda.graph on a capture stream) and replayed 3 times: every replay's y and dx
    follow that replay's mask, which is the eager mask of the same draw index."""
    seed, N = 9, 64
    l = _layer(0.5, seed, BF16)
    x = dev(torch.randn(N, 16, 2, 2, generator=torch.Generator().manual_seed(3)), BF16)
    dy = dev(torch.randn(N, 16, 2, 2, generator=torch.Generator().manual_seed(4)), BF16)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):  # warm-up: draws 1 and 2
            l.forward(x, 0)
            l.backward(dy, 0)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for t in l.step_state():
        t.zero_()  # roll the draw counter back, as TrainStep does with the state its warm-up touched
    g = torch.cuda.CUDAGraph()
    from dcnn_amd.runtime.capture import capture_guard
    with capture_guard(), torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
        y = l.forward(x, 0)
        dx = l.backward(dy, 0)
    masks = []
    e = _layer(0.5, seed, BF16)
    for k in range(3):
        g.replay()
        torch.cuda.synchronize()
        m = l.last_mask()
        masks.append(m.cpu())
        mv = m.view(-1, 1, 1, 1)
        assert torch.equal(m.cpu(), cpu_mask(seed, k + 1, N, 0.5))
        assert torch.equal(y, (x.float() * mv).to(BF16)) and torch.equal(dx, (dy.float() * mv).to(BF16))
        ye = e.forward(x, 0)
        dxe = e.backward(dy, 0)
        torch.cuda.synchronize()
        assert torch.equal(y, ye) and torch.equal(dx, dxe)
    assert not torch.equal(masks[0], masks[1]) and not torch.equal(masks[1], masks[2]) \
        and not torch.equal(masks[0], masks[2])
