"""Channel LayerNorm / LayerScale HIP kernels (lnorm.hip through ops.hip.ln_* / lscale_*) and GELU
(pool_act.hip through the activation factory) against PyTorch on the CPU in float64, on operands
already rounded to the compute type — the method of tests/test_gpu_dwconv.py.

Bounds (derived, not measured on the GPU). One bf16 rounding is at most 2^-8 relative, so the
per-element bound 2^-7 |ref| + 1e-5 is a 2x margin over a kernel that is exact fp32 arithmetic plus
one output rounding (the fp32-vs-fp64 deviation of these sums is ~1e-6); for dx the absolute term
scales with the row's largest gradient, 1e-5 max(1, max_row |ref|), because dx is a difference of
terms of that size. Relative L2 < 1e-2 is tests/test_gpu_kernels.py's kernel bound (the output
rounding alone gives ~2e-3). Saved statistics are fp32: relative L2 < 1e-5. dgamma / dbeta are fp32
sums of exact-in-fp32 products accumulated into gradients pre-filled with ones: relative L2 < 1e-4
against ref + 1. fp32 instances: relative L2 < 1e-4 throughout. The centred-variance test uses
x = 256 + N(0, 1) in fp32: a two-pass fp32 variance gives ~1.5e-5 relative L2 on y, E[x^2] - mean^2
gives ~4e-3, the bound is 1e-4.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CL = torch.channels_last
BF16 = torch.bfloat16
F32 = torch.float32
EPS = 1e-6

# (R, C) rows x channels, or (N, C, H, W) for the channels_last case
CASES = [
    (1, 8),         # one row, one vector
    (3, 40),        # 5 vectors, fewer rows than one wave holds
    (70, 96),       # 12 vectors (lane group padded to 16), a ragged last row group
    (257, 64),
    (33, 768),      # more than one vector per lane
    (5, 2048),      # the upper bound
    (20011, 64),    # every workgroup loops; more than one slab row
    (2, 24, 3, 5),  # 4-D channels_last
]
LOOPING = (20011, 64)
LSCALE_CASES = [(3, 40), (70, 96), (20011, 64)]
_id = lambda c: "x".join(str(v) for v in c)  # noqa: E731


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


def rows_of(case):
    return (case[0] * case[2] * case[3], case[1]) if len(case) == 4 else case


def as_rows(t, case):
    """[R, C] view of a reference tensor of the case's logical shape"""
    return t.permute(0, 2, 3, 1).reshape(-1, case[1]) if len(case) == 4 else t


def dev(t, case, dtype):
    t = t.to(dtype).cuda()
    return t.contiguous(memory_format=CL) if len(case) == 4 else t.contiguous()


_REF = {}


def reference(case, dtype, affine):
    """Operands (rounded to bf16 for the bf16 run) and the float64 CPU results, once per case."""
    key = (case, dtype, affine)
    if key in _REF:
        return _REF[key]
    R, C = rows_of(case)
    g = torch.Generator().manual_seed(4321)
    rnd = (lambda t: t.to(BF16).float()) if dtype == BF16 else (lambda t: t)
    shape = tuple(case)
    x, dy, res = (rnd(torch.randn(shape, generator=g)) for _ in range(3))
    gamma = 1.0 + 0.5 * torch.randn(C, generator=g)
    beta = torch.randn(C, generator=g)
    xr = as_rows(x, case).double().requires_grad_(True)
    gm = gamma.double().requires_grad_(True)
    bt = beta.double().requires_grad_(True)
    y = F.layer_norm(xr, (C,), gm if affine else None, bt if affine else None, EPS)
    y.backward(as_rows(dy, case).double())
    mean = xr.detach().mean(1)
    rstd = 1.0 / torch.sqrt(xr.detach().var(1, unbiased=False) + EPS)
    # LayerScale: y = gamma x (+ res), dx = gamma dy, dgamma = sum dy x
    xd, dyd = as_rows(x, case).double(), as_rows(dy, case).double()
    r = dict(x=x, dy=dy, res=res, gamma=gamma, beta=beta, y=y.detach(), dx=xr.grad, mean=mean, rstd=rstd,
             dgamma=gm.grad if affine else None, dbeta=bt.grad if affine else None,
             ls_y=gamma.double() * xd, ls_yres=gamma.double() * xd + as_rows(res, case).double(),
             ls_dx=gamma.double() * dyd, ls_dgamma=(dyd * xd).sum(0))
    _REF[key] = r
    return r


def run_ln(hip, case, dtype, affine):
    r = reference(case, dtype, affine)
    x, dy = dev(r["x"], case, dtype), dev(r["dy"], case, dtype)
    gamma = r["gamma"].cuda() if affine else None
    beta = r["beta"].cuda() if affine else None
    y, mean, rstd = hip.ln_fwd(x, gamma, beta, EPS)
    C = rows_of(case)[1]
    dg = torch.ones(C, device="cuda") if affine else None
    db = torch.ones(C, device="cuda") if affine else None
    dx = hip.ln_bwd(dy, x, gamma, mean, rstd, dg, db)
    torch.cuda.synchronize()
    assert y.dtype == dtype and dx.dtype == dtype and tuple(y.shape) == tuple(case) == tuple(dx.shape)
    if len(case) == 4:
        assert y.is_contiguous(memory_format=CL) and dx.is_contiguous(memory_format=CL)
    return r, as_rows(y, case), mean, rstd, as_rows(dx, case), dg, db


@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_ln_bf16(hip, case, affine):
    """(a) forward and (b) backward of the bf16 instances."""
    r, y, mean, rstd, dx, dg, db = run_ln(hip, case, BF16, affine)
    e, x = rel_err(y, r["y"]), elem_excess(y, r["y"])
    em, er = rel_err(mean, r["mean"]), rel_err(rstd, r["rstd"])
    print(f"fwd rel {e:.3e} elem {x:.3f} mean {em:.2e} rstd {er:.2e}")
    assert e < 1e-2 and x <= 1.0
    assert em < 1e-5 and er < 1e-5
    row_max = r["dx"].abs().amax(1, keepdim=True).clamp(min=1.0)
    e, x = rel_err(dx, r["dx"]), elem_excess(dx, r["dx"], 1e-5 * row_max)
    print(f"bwd dx rel {e:.3e} elem {x:.3f}")
    assert e < 1e-2 and x <= 1.0
    if affine:
        eg, eb = rel_err(dg, r["dgamma"] + 1), rel_err(db, r["dbeta"] + 1)
        print(f"dgamma {eg:.2e} dbeta {eb:.2e}")
        assert eg < 1e-4 and eb < 1e-4


@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_ln_fp32(hip, case, affine):
    """(c) the fp32 instances."""
    r, y, mean, rstd, dx, dg, db = run_ln(hip, case, F32, affine)
    errs = dict(y=rel_err(y, r["y"]), dx=rel_err(dx, r["dx"]), mean=rel_err(mean, r["mean"]),
                rstd=rel_err(rstd, r["rstd"]))
    if affine:
        errs.update(dgamma=rel_err(dg, r["dgamma"] + 1), dbeta=rel_err(db, r["dbeta"] + 1))
    print(" ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v < 1e-4 for v in errs.values())


def test_partial_rows(hip):
    from dcnn_amd.ops._ext import kernels
    K = kernels()
    assert K.ln_partial_rows(*LOOPING) > 1  # the slab reduce sums more than one row in that case
    assert K.ln_partial_rows(1, 8) == 1
    assert K.ln_workspace_bytes(*LOOPING) == K.ln_partial_rows(*LOOPING) * 2 * LOOPING[1] * 4
    assert K.ln_supported(1, 70, 96) and K.ln_supported(0, 70, 12)
    assert not K.ln_supported(1, 70, 12) and not K.ln_supported(0, 70, 4096) and not K.ln_supported(1, 70, 4)
    assert not K.ln_supported(1, 1 << 22, 512)  # 2^31 elements


@pytest.mark.parametrize("C", [96, 768])
def test_ln_centred_variance(hip, C):
    """(d) a large common offset: E[x^2] - mean^2 in fp32 loses the variance, the centred sum keeps it."""
    g = torch.Generator().manual_seed(7)
    x = 256.0 + torch.randn(70, C, generator=g)
    ref = F.layer_norm(x.double(), (C,), None, None, EPS)
    y, _, _ = hip.ln_fwd(x.cuda(), None, None, EPS)
    e = rel_err(y, ref)
    print(f"C={C} rel {e:.3e}")
    assert e < 1e-4


def test_bwd_deterministic(hip):
    """(e) the parameter gradients of two runs from the same inputs are the same bits."""
    case = LOOPING
    C = case[1]
    r = reference(case, BF16, True)
    x, dy = dev(r["x"], case, BF16), dev(r["dy"], case, BF16)
    gamma, beta = r["gamma"].cuda(), r["beta"].cuda()
    _, mean, rstd = hip.ln_fwd(x, gamma, beta, EPS)
    outs = []
    for _ in range(2):
        dg, db, dls = (torch.zeros(C, device="cuda") for _ in range(3))
        hip.ln_bwd(dy, x, gamma, mean, rstd, dg, db)
        hip.lscale_bwd(dy, x, gamma, dls)
        torch.cuda.synchronize()
        outs.append((dg.cpu(), db.cpu(), dls.cpu()))
    for a, b in zip(*outs):
        assert a.abs().sum() > 0 and torch.equal(a, b)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("case", LSCALE_CASES, ids=_id)
def test_lscale(hip, case, residual, dtype):
    """(f) LayerScale forward (+ residual) and backward."""
    r = reference(case, dtype, True)
    x, dy = dev(r["x"], case, dtype), dev(r["dy"], case, dtype)
    gamma = r["gamma"].cuda()
    y = hip.lscale_fwd(x, gamma, dev(r["res"], case, dtype) if residual else None)
    dg = torch.ones(case[1], device="cuda")
    dx = hip.lscale_bwd(dy, x, gamma, dg)
    torch.cuda.synchronize()
    yref = r["ls_yres"] if residual else r["ls_y"]
    assert y.dtype == dtype and dx.dtype == dtype and tuple(y.shape) == tuple(case) == tuple(dx.shape)
    ey, ex, eg = rel_err(y, yref), rel_err(dx, r["ls_dx"]), rel_err(dg, r["ls_dgamma"] + 1)
    print(f"y {ey:.3e} dx {ex:.3e} dgamma {eg:.2e}")
    if dtype == F32:
        assert ey < 1e-4 and ex < 1e-4 and eg < 1e-4
        return
    xy, xx = elem_excess(y, yref), elem_excess(dx, r["ls_dx"])
    print(f"elem y {xy:.3f} dx {xx:.3f}")
    assert ey < 1e-2 and xy <= 1.0
    assert ex < 1e-2 and xx <= 1.0
    assert eg < 1e-4


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
def test_gelu(hip, dtype):
    """(g) exact GELU and its gradient through the activation factory."""
    from dcnn_amd.nn.activations import ActivationFactory
    act = ActivationFactory.create("gelu")
    g = torch.Generator().manual_seed(11)
    x = torch.linspace(-8.0, 8.0, 4099)
    x[0], x[2049], x[-1] = -8.0, 0.0, 8.0
    dy = torch.randn(4099, generator=g)
    if dtype == BF16:
        x, dy = x.to(BF16).float(), dy.to(BF16).float()
    assert (x == 0).any() and x.min() == -8 and x.max() == 8
    xd = x.double().requires_grad_(True)
    ref = F.gelu(xd)
    ref.backward(dy.double())
    xg = x.to(dtype).cuda()
    y = act.apply(xg)
    dx = act.gradient(xg, y, dy.to(dtype).cuda())
    torch.cuda.synchronize()
    assert y.dtype == dtype and dx.dtype == dtype
    if dtype == BF16:
        ey, ex = elem_excess(y, ref.detach()), elem_excess(dx, xd.grad)
        print(f"elem y {ey:.3f} dx {ex:.3f}")
        assert ey <= 1.0 and ex <= 1.0
    else:
        ey, ex = rel_err(y, ref.detach()), rel_err(dx, xd.grad)
        print(f"rel y {ey:.3e} dx {ex:.3e}")
        assert ey < 1e-5 and ex < 1e-5


def test_unsupported_shapes(hip):
    """(h) a shape outside the supported set is an error that names it."""
    x = torch.zeros(16, 12, device="cuda", dtype=BF16)
    with pytest.raises(ValueError, match=r"\(16, 12\)"):
        hip.ln_fwd(x, None, None, EPS)
    with pytest.raises(ValueError, match=r"\(16, 12\)"):
        hip.lscale_fwd(x, torch.ones(12, device="cuda"))
    for dtype in (BF16, F32):
        x = torch.zeros(4, 4096, device="cuda", dtype=dtype)
        with pytest.raises(ValueError, match="4096"):
            hip.ln_fwd(x, None, None, EPS)
        with pytest.raises(ValueError, match="4096"):
            hip.ln_bwd(x, x, None, torch.zeros(4, device="cuda"), torch.ones(4, device="cuda"), None, None)
