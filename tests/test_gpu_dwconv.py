"""Depthwise-conv HIP kernels (dwconv.hip through ops.hip.dwconv2d_*) against PyTorch fp32 on the
CPU — F.conv2d(groups=C) and torch.nn.grad.conv2d_input / conv2d_weight(groups=C) on bf16-rounded
operands, the yardstick of tests/test_gpu_kernels.py.

Bounds. fwd / dgrad: relative L2 < 1e-2 (that file's kernel bound; the bf16 output rounding alone
gives ~1.7e-3) and, per element, |y - y_ref| <= 2^-7 |y_ref| + 1e-5 — one bf16 rounding is at most
2^-8 relative and the fp32 accumulation of <= 49 exact products ~1e-6 absolute, a 2x margin; the L2
check alone would let a single wrong border pixel through. wgrad (into gradients pre-filled with
ones): relative L2 < 1e-4 — products of bf16 operands are exact in fp32, only the summation order
differs. fp32 instances: relative L2 < 1e-4 for all three passes.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CL = torch.channels_last
BF16 = torch.bfloat16

# (N, C, H, W, (KH, KW), (SH, SW), (PH, PW))
CASES = [
    (1, 8, 1, 1, (3, 3), (1, 1), (1, 1)),      # one pixel, one channel vector: all taps but the centre are padding
    (2, 32, 2, 2, (3, 3), (2, 2), (1, 1)),     # output 1x1
    (2, 64, 16, 16, (3, 3), (1, 1), (1, 1)),   # compile-time s1 instance, several x-runs per row
    (2, 64, 16, 16, (3, 3), (2, 2), (1, 1)),   # compile-time s2 instance
    (3, 40, 7, 5, (3, 3), (1, 1), (1, 1)),     # 5 channel vectors, odd map narrower than one run, N = 3
    (3, 40, 7, 5, (3, 3), (2, 2), (1, 1)),     # s2 on an odd map: 4x3 output
    (2, 16, 8, 8, (3, 3), (2, 2), (0, 0)),     # (H - KH) % SH != 0: input row / column 7 unused
    (4, 512, 4, 4, (3, 3), (1, 1), (1, 1)),    # wide and tiny: every pixel on a border
    (2, 128, 9, 9, (3, 3), (2, 2), (1, 1)),    # 5x5 output
    (2, 32, 8, 8, (3, 3), (1, 1), (0, 0)),     # pad 0 -> run-time instance
    (2, 24, 12, 10, (5, 5), (1, 1), (2, 2)),   # run-time instance, 25 taps (three wgrad tap groups)
    (2, 16, 9, 9, (7, 7), (2, 2), (3, 3)),     # 49 taps, s2
    (2, 16, 10, 6, (1, 3), (1, 2), (0, 1)),    # rectangular kernel, stride and pad
    (64, 256, 8, 8, (3, 3), (1, 1), (1, 1)),   # weight gradient over more than one split
]
MULTI_SPLIT = CASES[-1]
_ids = [f"n{c[0]}c{c[1]}_{c[2]}x{c[3]}_k{c[4][0]}x{c[4][1]}_s{c[5][0]}{c[5][1]}_p{c[6][0]}{c[6][1]}" for c in CASES]


def rel_err(a, b):
    a = a.float().cpu()
    b = b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def elem_excess(y, ref):
    """max over elements of |y - ref| / (2^-7 |ref| + 1e-5): <= 1 passes."""
    y = y.float().cpu()
    return ((y - ref).abs() / (ref.abs() * 2.0 ** -7 + 1e-5)).max().item()


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
    N, C, H, W, (KH, KW), st, pd = case
    g = torch.Generator().manual_seed(1234)
    rnd = (lambda t: t.to(BF16).float()) if dtype == BF16 else (lambda t: t)
    x = rnd(torch.randn(N, C, H, W, generator=g))
    w = rnd(torch.randn(C, 1, KH, KW, generator=g) / (KH * KW) ** 0.5)
    b = torch.randn(C, generator=g)
    y = F.conv2d(x, w, None, st, pd, groups=C)
    dy = rnd(torch.randn(y.shape, generator=g))
    res = rnd(torch.randn(N, C, H, W, generator=g))
    r = dict(x=x, w=w, b=b, dy=dy, res=res, y=y, yb=y + b.view(1, C, 1, 1),
             dx=torch.nn.grad.conv2d_input(x.shape, w, dy, st, pd, groups=C),
             dw=torch.nn.grad.conv2d_weight(x, w.shape, dy, st, pd, groups=C), db=dy.sum((0, 2, 3)))
    _REF[key] = r
    return r


def act(t, dtype):
    return t.cuda().to(dtype).contiguous(memory_format=CL)


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_dwconv_fwd(hip, case, bias):
    r = reference(case, BF16)
    st, pd = case[5], case[6]
    y = hip.dwconv2d_fwd(act(r["x"], BF16), r["w"].cuda().to(BF16), r["b"].cuda() if bias else None, st, pd)
    ref = r["yb"] if bias else r["y"]
    assert y.dtype == BF16 and tuple(y.shape) == tuple(ref.shape) and y.is_contiguous(memory_format=CL)
    e, x = rel_err(y, ref), elem_excess(y, ref)
    print(f"fwd rel {e:.3e} elem {x:.3f}")
    assert e < 1e-2
    assert x <= 1.0


@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_dwconv_dgrad(hip, case, residual):
    r = reference(case, BF16)
    st, pd = case[5], case[6]
    dx = hip.dwconv2d_dgrad(act(r["dy"], BF16), r["w"].cuda().to(BF16), tuple(r["x"].shape), st, pd,
                            residual=act(r["res"], BF16) if residual else None)
    ref = r["dx"] + r["res"] if residual else r["dx"]
    assert dx.dtype == BF16 and tuple(dx.shape) == tuple(ref.shape) and dx.is_contiguous(memory_format=CL)
    e, x = rel_err(dx, ref), elem_excess(dx, ref)
    print(f"dgrad rel {e:.3e} elem {x:.3f}")
    assert e < 1e-2
    assert x <= 1.0


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_dwconv_wgrad(hip, case, bias):
    r = reference(case, BF16)
    N, C, H, W, (KH, KW), st, pd = case
    gw = torch.ones(C, 1, KH, KW, device="cuda")
    gb = torch.ones(C, device="cuda") if bias else None
    hip.dwconv2d_wgrad(act(r["dy"], BF16), act(r["x"], BF16), (C, 1, KH, KW), st, pd, gw, gb)
    e = rel_err(gw, r["dw"] + 1)
    print(f"wgrad rel {e:.3e}")
    assert e < 1e-4
    if bias:
        eb = rel_err(gb, r["db"] + 1)
        print(f"bias grad rel {eb:.3e}")
        assert eb < 1e-4


@pytest.mark.parametrize("case", CASES[:7], ids=_ids[:7])
def test_dwconv_fp32(hip, case):
    r = reference(case, torch.float32)
    N, C, H, W, (KH, KW), st, pd = case
    F32 = torch.float32
    w = r["w"].cuda()
    y = hip.dwconv2d_fwd(act(r["x"], F32), w, r["b"].cuda(), st, pd)
    dx = hip.dwconv2d_dgrad(act(r["dy"], F32), w, tuple(r["x"].shape), st, pd, residual=act(r["res"], F32))
    gw = torch.ones(C, 1, KH, KW, device="cuda")
    gb = torch.ones(C, device="cuda")
    hip.dwconv2d_wgrad(act(r["dy"], F32), act(r["x"], F32), (C, 1, KH, KW), st, pd, gw, gb)
    errs = (rel_err(y, r["yb"]), rel_err(dx, r["dx"] + r["res"]), rel_err(gw, r["dw"] + 1), rel_err(gb, r["db"] + 1))
    print("fp32 fwd / dgrad / wgrad / bias rel", " ".join(f"{e:.3e}" for e in errs))
    assert y.dtype == F32 and dx.dtype == F32
    assert max(errs) < 1e-4


def test_dwconv_multi_split_deterministic(hip):
    r = reference(MULTI_SPLIT, BF16)
    N, C, H, W, (KH, KW), st, pd = MULTI_SPLIT
    assert hip.dwconv_wgrad_splits(BF16, (N, C, H, W), (C, 1, KH, KW), st, pd) > 1
    x, dy, w = act(r["x"], BF16), act(r["dy"], BF16), r["w"].cuda().to(BF16)

    def run():
        y = hip.dwconv2d_fwd(x, w, None, st, pd)
        dx = hip.dwconv2d_dgrad(dy, w, (N, C, H, W), st, pd)
        gw = torch.zeros(C, 1, KH, KW, device="cuda")
        gb = torch.zeros(C, device="cuda")
        hip.dwconv2d_wgrad(dy, x, (C, 1, KH, KW), st, pd, gw, gb)
        return y.clone(), dx.clone(), gw, gb

    for a, b in zip(run(), run()):
        assert torch.equal(a, b)


def test_dwconv_unsupported_shapes_raise(hip):
    x = torch.zeros(2, 12, 8, 8, device="cuda", dtype=BF16).contiguous(memory_format=CL)
    w = torch.zeros(12, 1, 3, 3, device="cuda", dtype=BF16)
    with pytest.raises(ValueError, match=r"C=12.*3x3"):
        hip.dwconv2d_fwd(x, w, None, (1, 1), (1, 1))
    with pytest.raises(ValueError, match=r"C=12"):
        hip.dwconv2d_dgrad(x, w, (2, 12, 8, 8), (1, 1), (1, 1))
    with pytest.raises(ValueError, match=r"C=12"):
        hip.dwconv2d_wgrad(x, x, (12, 1, 3, 3), (1, 1), (1, 1), torch.zeros(12, 1, 3, 3, device="cuda"))
    x = torch.zeros(2, 16, 12, 12, device="cuda", dtype=BF16).contiguous(memory_format=CL)
    w = torch.zeros(16, 1, 8, 8, device="cuda", dtype=BF16)
    with pytest.raises(ValueError, match=r"C=16.*8x8"):
        hip.dwconv2d_fwd(x, w, None, (1, 1), (0, 0))
