"""Grouped-conv HIP kernels (gconv.hip through ops.hip.gconv2d_*) against PyTorch fp32 on the CPU —
F.conv2d(groups=G) and torch.nn.grad.conv2d_input / conv2d_weight(groups=G) on bf16-rounded
operands, the method of tests/test_gpu_dwconv.py. Operands: seed 1234, w ~ randn / sqrt(Cig KH KW).

Bounds. fwd / dgrad (bf16): relative L2 < 1e-2 (the project's kernel bound) and, per element,
|y - ref| <= 2^-7 |ref| + 2 K 2^-24 A, with A the same convolution of the absolute values of the
operands (+ |residual|) and K the reduction length (Cig KH KW forward, Cog KH KW dgrad): one bf16
rounding is at most 2^-8 relative and the fp32 accumulation of K terms in any order at most
K 2^-24 sum |a b|, each with a 2x margin. wgrad (into gradients pre-filled with ones): relative
L2 < 1e-4 for dW and db — products of bf16 operands are exact in fp32, only the order differs.
fp32 instances: relative L2 < 1e-4 for all three passes.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CL = torch.channels_last
BF16 = torch.bfloat16

# (N, Ci, Co, G, H, W, (KH, KW), (SH, SW), (PH, PW))
CASES = [
    (1, 8, 16, 2, 1, 1, (3, 3), (1, 1), (1, 1)),       # one pixel; Cig 4, Cog 8; all taps but the centre are padding
    (2, 32, 32, 8, 5, 7, (3, 3), (1, 1), (1, 1)),      # Cig = Cog = 4, four-group bundles, map smaller than a tile
    (2, 64, 64, 8, 16, 16, (3, 3), (1, 1), (1, 1)),    # Cig 8, four taps per k-step
    (2, 64, 64, 4, 9, 9, (3, 3), (2, 2), (1, 1)),      # Cig 16, stride 2 on an odd map, 5x5 output
    (2, 64, 128, 2, 8, 8, (3, 3), (1, 1), (1, 1)),     # Cig 32, Cog 64, Ci != Co
    (1, 128, 128, 2, 6, 6, (3, 3), (1, 1), (1, 1)),    # Cig 64, two k-steps per tap
    (2, 256, 256, 2, 4, 4, (3, 3), (1, 1), (1, 1)),    # Cig 128; every pixel on a border
    (2, 48, 96, 3, 7, 5, (3, 3), (2, 2), (1, 1)),      # G = 3, Cig 16, Cog 32
    (2, 24, 24, 3, 8, 8, (3, 3), (1, 1), (1, 1)),      # G = 3 with two-group bundles; last bundle half empty
    (2, 64, 32, 4, 8, 8, (1, 1), (1, 1), (0, 0)),      # grouped pointwise; Cog 8 < Cig 16
    (2, 32, 32, 4, 10, 6, (5, 5), (1, 1), (2, 2)),     # 25 taps
    (2, 16, 32, 2, 10, 6, (1, 3), (1, 2), (0, 1)),     # rectangular kernel, stride and pad
    (2, 32, 32, 4, 8, 8, (3, 3), (2, 2), (0, 0)),      # (H - KH) % S != 0: last input row and column unused
    (32, 128, 128, 32, 8, 8, (3, 3), (1, 1), (1, 1)),  # weight gradient over more than one split
]
MULTI_SPLIT = CASES[-1]
_ids = [f"n{c[0]}c{c[1]}o{c[2]}g{c[3]}_{c[4]}x{c[5]}_k{c[6][0]}x{c[6][1]}_s{c[7][0]}{c[7][1]}_p{c[8][0]}{c[8][1]}"
        for c in CASES]


def rel_err(a, b):
    a = a.float().cpu()
    b = b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def elem_excess(y, ref, A, K):
    """max over elements of |y - ref| / (2^-7 |ref| + 2 K 2^-24 A): <= 1 passes."""
    err = (y.float().cpu() - ref).abs()
    bound = ref.abs() * 2.0 ** -7 + 2.0 * K * 2.0 ** -24 * A
    # an input pixel no output reaches has ref = A = 0: the bound is 0 and only an exact 0 meets it
    zero = torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err))
    return torch.where(bound > 0, err / bound, zero).max().item()


@pytest.fixture(scope="module")
def hip():
    from dcnn_amd.ops import hip as h
    from dcnn_amd.ops._ext import kernels
    assert kernels().arch == "gfx950"
    return h


_REF = {}


def reference(case, dtype):
    """Operands (rounded to bf16 for the bf16 run) and the CPU fp32 results, computed once per case."""
    key = (case, dtype)
    if key in _REF:
        return _REF[key]
    N, Ci, Co, G, H, W, (KH, KW), st, pd = case
    Cig = Ci // G
    g = torch.Generator().manual_seed(1234)
    rnd = (lambda t: t.to(BF16).float()) if dtype == BF16 else (lambda t: t)
    x = rnd(torch.randn(N, Ci, H, W, generator=g))
    w = rnd(torch.randn(Co, Cig, KH, KW, generator=g) / (Cig * KH * KW) ** 0.5)
    b = torch.randn(Co, generator=g)
    y = F.conv2d(x, w, None, st, pd, groups=G)
    dy = rnd(torch.randn(y.shape, generator=g))
    res = rnd(torch.randn(N, Ci, H, W, generator=g))
    r = dict(x=x, w=w, b=b, dy=dy, res=res, y=y, yb=y + b.view(1, Co, 1, 1),
             ya=F.conv2d(x.abs(), w.abs(), None, st, pd, groups=G),
             dx=torch.nn.grad.conv2d_input(x.shape, w, dy, st, pd, groups=G),
             dxa=torch.nn.grad.conv2d_input(x.shape, w.abs(), dy.abs(), st, pd, groups=G),
             dw=torch.nn.grad.conv2d_weight(x, w.shape, dy, st, pd, groups=G), db=dy.sum((0, 2, 3)))
    _REF[key] = r
    return r


def act(t, dtype):
    return t.cuda().to(dtype).contiguous(memory_format=CL)


def ones_w(Co, Cig, KH, KW):
    return torch.ones(Co, Cig, KH, KW, device="cuda").contiguous(memory_format=CL)


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_gconv_fwd(hip, case, bias):
    r = reference(case, BF16)
    N, Ci, Co, G, H, W, (KH, KW), st, pd = case
    y = hip.gconv2d_fwd(act(r["x"], BF16), act(r["w"], BF16), r["b"].cuda() if bias else None, st, pd, G)
    ref = r["yb"] if bias else r["y"]
    assert y.dtype == BF16 and tuple(y.shape) == tuple(ref.shape) and y.is_contiguous(memory_format=CL)
    e, x = rel_err(y, ref), elem_excess(y, ref, r["ya"], Ci // G * KH * KW)
    print(f"fwd rel {e:.3e} elem {x:.3f}")
    assert e < 1e-2
    assert x <= 1.0


@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_gconv_dgrad(hip, case, residual):
    r = reference(case, BF16)
    N, Ci, Co, G, H, W, (KH, KW), st, pd = case
    dx = hip.gconv2d_dgrad(act(r["dy"], BF16), act(r["w"], BF16), tuple(r["x"].shape), st, pd, G,
                           residual=act(r["res"], BF16) if residual else None)
    ref = r["dx"] + r["res"] if residual else r["dx"]
    A = r["dxa"] + r["res"].abs() if residual else r["dxa"]
    assert dx.dtype == BF16 and tuple(dx.shape) == tuple(ref.shape) and dx.is_contiguous(memory_format=CL)
    e, x = rel_err(dx, ref), elem_excess(dx, ref, A, Co // G * KH * KW)
    print(f"dgrad rel {e:.3e} elem {x:.3f}")
    assert e < 1e-2
    assert x <= 1.0


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_gconv_wgrad(hip, case, bias):
    r = reference(case, BF16)
    N, Ci, Co, G, H, W, (KH, KW), st, pd = case
    Cig = Ci // G
    gw = ones_w(Co, Cig, KH, KW)
    gb = torch.ones(Co, device="cuda") if bias else None
    hip.gconv2d_wgrad(act(r["dy"], BF16), act(r["x"], BF16), (Co, Cig, KH, KW), st, pd, G, gw, gb)
    e = rel_err(gw, r["dw"] + 1)
    print(f"wgrad rel {e:.3e}")
    assert e < 1e-4
    if bias:
        eb = rel_err(gb, r["db"] + 1)
        print(f"bias grad rel {eb:.3e}")
        assert eb < 1e-4


@pytest.mark.parametrize("case", CASES[:8], ids=_ids[:8])
def test_gconv_fp32(hip, case):
    r = reference(case, torch.float32)
    N, Ci, Co, G, H, W, (KH, KW), st, pd = case
    Cig = Ci // G
    F32 = torch.float32
    w = act(r["w"], F32)
    y = hip.gconv2d_fwd(act(r["x"], F32), w, r["b"].cuda(), st, pd, G)
    dx = hip.gconv2d_dgrad(act(r["dy"], F32), w, tuple(r["x"].shape), st, pd, G, residual=act(r["res"], F32))
    gw = ones_w(Co, Cig, KH, KW)
    gb = torch.ones(Co, device="cuda")
    hip.gconv2d_wgrad(act(r["dy"], F32), act(r["x"], F32), (Co, Cig, KH, KW), st, pd, G, gw, gb)
    errs = (rel_err(y, r["yb"]), rel_err(dx, r["dx"] + r["res"]), rel_err(gw, r["dw"] + 1), rel_err(gb, r["db"] + 1))
    print("fp32 fwd / dgrad / wgrad / bias rel", " ".join(f"{e:.3e}" for e in errs))
    assert y.dtype == F32 and dx.dtype == F32
    assert max(errs) < 1e-4


def test_gconv_multi_split_deterministic(hip):
    r = reference(MULTI_SPLIT, BF16)
    N, Ci, Co, G, H, W, (KH, KW), st, pd = MULTI_SPLIT
    Cig = Ci // G
    assert hip.gconv_wgrad_splits(BF16, (N, Ci, H, W), (Co, Cig, KH, KW), st, pd, G) > 1
    x, dy, w = act(r["x"], BF16), act(r["dy"], BF16), act(r["w"], BF16)

    def run():
        y = hip.gconv2d_fwd(x, w, None, st, pd, G)
        dx = hip.gconv2d_dgrad(dy, w, (N, Ci, H, W), st, pd, G)
        gw = torch.zeros(Co, Cig, KH, KW, device="cuda").contiguous(memory_format=CL)
        gb = torch.zeros(Co, device="cuda")
        hip.gconv2d_wgrad(dy, x, (Co, Cig, KH, KW), st, pd, G, gw, gb)
        return y.clone(), dx.clone(), gw, gb

    for a, b in zip(run(), run()):
        assert torch.equal(a, b)


def test_gconv_matches_dense_block_diagonal(hip):
    """The project's dense conv2d_fwd on the block-diagonal expansion of the same weights: both are
    rounded once from fp32 sums taken in different orders."""
    case = (2, 64, 64, 4, 8, 8, (3, 3), (1, 1), (1, 1))
    N, Ci, Co, G, H, W, (KH, KW), st, pd = case
    Cig, Cog = Ci // G, Co // G
    r = reference(case, BF16)
    wd = torch.zeros(Co, Ci, KH, KW)
    for g in range(G):
        wd[g * Cog:(g + 1) * Cog, g * Cig:(g + 1) * Cig] = r["w"][g * Cog:(g + 1) * Cog]
    x = act(r["x"], BF16)
    y = hip.gconv2d_fwd(x, act(r["w"], BF16), r["b"].cuda(), st, pd, G)
    yd, _ = hip.conv2d_fwd(x, act(wd, BF16), r["b"].cuda(), st, pd)
    e = rel_err(y, yd)
    print(f"grouped vs dense block-diagonal rel {e:.3e}")
    assert e < 5e-3


def test_gconv_unsupported_shapes_raise(hip):
    def zeros(*s, dtype=BF16):
        return torch.zeros(*s, device="cuda", dtype=dtype).contiguous(memory_format=CL)

    def all_three(N, Ci, Co, G, H, W, KH, KW, pad, match):
        Cig = max(Ci // G, 1)
        OH, OW = H + 2 * pad - KH + 1, W + 2 * pad - KW + 1
        x, dy, w = zeros(N, Ci, H, W), zeros(N, Co, OH, OW), zeros(Co, Cig, KH, KW)
        with pytest.raises(ValueError, match=match):
            hip.gconv2d_fwd(x, w, None, (1, 1), (pad, pad), G)
        with pytest.raises(ValueError, match=match):
            hip.gconv2d_dgrad(dy, w, (N, Ci, H, W), (1, 1), (pad, pad), G)
        with pytest.raises(ValueError, match=match):
            hip.gconv2d_wgrad(dy, x, (Co, Cig, KH, KW), (1, 1), (pad, pad), G, zeros(Co, Cig, KH, KW, dtype=torch.float32))

    all_three(2, 24, 24, 2, 8, 8, 3, 3, 1, r"Ci=24.*G=2.*Cig=12.*3x3")   # Cig = 12
    all_three(2, 8, 8, 8, 8, 8, 3, 3, 1, r"Ci=8.*G=8.*Cig=1")            # Cig = Cog = 1 (depthwise)
    all_three(2, 16, 16, 2, 12, 12, 8, 8, 0, r"Ci=16.*G=2.*8x8")         # 64 taps
    all_three(2, 20, 16, 8, 8, 8, 3, 3, 1, r"Ci=20.*G=8")                # Ci % G != 0
