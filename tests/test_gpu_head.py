"""The fused classifier-head kernels (csrc/kernels/head.hip through the raw bindings): head_fwd =
global average pool + FC + bias, head_bwd = FC data gradient + pool backward + FC weight / bias
gradients, against an fp64 reference and against today's separate kernels on the same inputs.

Reference: torch on the CPU in fp64 from the same bf16 inputs, rounded to bf16 where both GPU paths
round: the pooled value, the logits, the pooled gradient, and dx. The backward gets random bf16
dlogits (and the reference's pooled tile), so it does not depend on the forward.

Criterion per output, both errors printed: the fused kernels' relative L2 error against the
reference is at most 1.5 x that of the separate kernels (avgpool_fwd + gemm_nt; conv_weight_transpose
+ gemm_nt + avgpool_bwd; gemm_tn + splitk_reduce2) plus 2^-8 (one bf16 unit of the reference's RMS)
for the bf16 outputs, plus 1e-6 for the fp32 gradients. Both paths round at the same points, so the
ratio is about 1; 1.5 absorbs a different fp32 summation order. The kernels are built to do better:
they keep the separate kernels' summation order, so each output is also required to be bit-identical
to the separate path's (a training run then computes what it computed before). Every output buffer is pre-filled
with a sentinel and carries a sentinel tail: nothing past row N (or past class Out of the last row)
may be written and everything before must be. Two runs are bit-identical.

Shapes (N, HW, In, Out): the smallest at which each mechanism can fail — partial image blocks,
partial class tiles, a single k-block, the LDS maximum (In = 2048), HW = 1; then the sizes at which
the launchers take another path: 8 and 16 images per forward workgroup (N > 248 / N > 496), more than
one batch split of the weight blocks with a partial last split (N = 300), and more classes than
the data blocks stage in one pass (Out > 256)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
SENT = -777.0
TAIL = 4096

# (N, (H, W), In, Out)
CASES = [
    (1, (1, 1), 64, 7),        # smallest everything
    (17, (4, 4), 512, 200),    # partial image block, the real head shape
    (40, (2, 2), 64, 10),      # several blocks, Out < 16
    (16, (8, 8), 128, 33),     # 8 x 8 map, odd class count
    (19, (4, 4), 2048, 200),   # ResNet-50's width at the LDS bound
    (300, (1, 1), 64, 7),      # 8 images per forward workgroup; 4 batch splits of 128: two chunks, a partial and an empty split
    (520, (1, 1), 64, 7),      # 16 images per forward workgroup, partial last block
    (16, (1, 1), 64, 300),     # two class passes in the data blocks, the second one partial
]
_ids = [f"n{c[0]}_{c[1][0]}x{c[1][1]}_i{c[2]}_o{c[3]}" for c in CASES]


@pytest.fixture(scope="module")
def K():
    from dcnn_amd.ops._ext import kernels
    k = kernels()
    assert k.arch == "gfx950"
    return k


def _st():
    return torch.cuda.current_stream().cuda_stream


_REF = {}


def reference(case):
    """bf16 inputs and the fp64 results (rounded where the kernels round), once per case."""
    if case in _REF:
        return _REF[case]
    N, (H, W), In, Out = case
    HW = H * W
    g = torch.Generator().manual_seed(4321)
    x = torch.randn(N, HW, In, generator=g).to(BF16)
    w = (torch.randn(Out, In, generator=g) / In ** 0.5).to(BF16)
    b = torch.randn(Out, generator=g) * 0.1
    dl = (torch.randn(N, Out, generator=g) / N).to(BF16)
    pooled = (x.double().sum(1) / HW).to(BF16)
    logits = (pooled.double() @ w.double().t() + b.double()).to(BF16)
    dpooled = (dl.double() @ w.double()).to(BF16)
    dx = (dpooled.double() / HW).to(BF16).view(N, 1, In).expand(N, HW, In).contiguous()
    r = dict(x=x, w=w, b=b, dl=dl, pooled=pooled, logits=logits, dx=dx, dw=dl.double().t() @ pooled.double(),
             db=dl.double().sum(0))
    _REF[case] = r
    return r


def geom(case):
    N, (H, W), In, Out = case
    return (N, H, W, In, 1, 1, H, W, 1, 1, 0, 0)


def buf(n, dtype):
    """n elements to write, then a sentinel tail; everything pre-filled with the sentinel."""
    return torch.full((n + TAIL,), SENT, dtype=dtype, device="cuda")


def taken(t, n, shape):
    """The written part, after checking the tail is untouched and nothing before it was left out."""
    torch.cuda.synchronize()
    assert bool((t[n:] == SENT).all()), "wrote past the end of the buffer"
    body = t[:n]
    assert not bool((body == SENT).any()), "left part of the output unwritten"
    return body.view(shape).cpu()


def rel(a, ref):
    ref = ref.double()
    return float((a.double() - ref).norm() / ref.norm().clamp_min(1e-300))


def check(name, fused, unfused, ref, slack):
    ef, eu = rel(fused, ref), rel(unfused, ref)
    print(f"{name}: fused rel-L2 {ef:.3e}, separate kernels rel-L2 {eu:.3e}, bound {1.5 * eu + slack:.3e}")
    assert ef <= 1.5 * eu + slack, (name, ef, eu)
    # beyond the bound: the fused kernels run the separate kernels' MFMA chains (one accumulator,
    # 32 reduction elements per MFMA in ascending order, gemm_tn's batch split and bias-sum order)
    # and round at the same points, so every output is the separate path's bits
    assert torch.equal(fused, unfused), (name, float((fused.double() - unfused.double()).abs().max()))


def run_fwd_fused(K, case, d):
    N, _, In, Out = case
    pooled, logits = buf(N * In, BF16), buf(N * Out, BF16)
    K.head_fwd(d["x"].data_ptr(), d["w"].data_ptr(), d["b"].data_ptr(), pooled.data_ptr(), logits.data_ptr(),
               *geom(case), Out, _st())
    return taken(pooled, N * In, (N, In)), taken(logits, N * Out, (N, Out))


def run_fwd_separate(K, case, d):
    from dcnn_amd.ops.hip_base import PLAIN
    N, _, In, Out = case
    pooled, logits = buf(N * In, BF16), buf(N * Out, BF16)
    K.avgpool_fwd(1, d["x"].data_ptr(), pooled.data_ptr(), *geom(case), _st())
    K.gemm_nt(pooled.data_ptr(), d["w"].data_ptr(), logits.data_ptr(), N, Out, In, In, In, Out, PLAIN,
              0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 0, 0, d["b"].data_ptr(), 0, 0, 0, 0, _st())
    return taken(pooled, N * In, (N, In)), taken(logits, N * Out, (N, Out))


def _reduced(K, slab, bslab, splits, In, Out):
    dw, db = buf(Out * In, torch.float32), buf(Out, torch.float32)
    K.splitk_reduce2(slab.data_ptr(), dw.data_ptr(), Out * In, bslab.data_ptr(), db.data_ptr(), Out, splits, 0, _st())
    return taken(dw, Out * In, (Out, In)), taken(db, Out, (Out,))


def run_bwd_fused(K, case, d):
    N, (H, W), In, Out = case
    splits = K.head_bwd_splits(N, In, Out)
    dx = buf(N * H * W * In, BF16)
    slab, bslab = buf(splits * Out * In, torch.float32), buf(splits * Out, torch.float32)
    K.head_bwd(d["dl"].data_ptr(), d["w"].data_ptr(), d["pooled"].data_ptr(), dx.data_ptr(), slab.data_ptr(),
               bslab.data_ptr(), *geom(case), Out, _st())
    dxo = taken(dx, N * H * W * In, (N, H * W, In))
    taken(slab, splits * Out * In, (splits, Out, In))
    taken(bslab, splits * Out, (splits, Out))
    return (dxo,) + _reduced(K, slab, bslab, splits, In, Out)


def run_bwd_separate(K, case, d):
    from dcnn_amd.ops.hip_base import PLAIN
    N, (H, W), In, Out = case
    wt = torch.empty(In, Out, dtype=BF16, device="cuda")
    dpooled, dx = buf(N * In, BF16), buf(N * H * W * In, BF16)
    K.conv_weight_transpose(1, d["w"].data_ptr(), wt.data_ptr(), Out, 1, In, _st())
    K.gemm_nt(d["dl"].data_ptr(), wt.data_ptr(), dpooled.data_ptr(), N, In, Out, Out, Out, In, PLAIN,
              0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, _st())
    K.avgpool_bwd(1, dpooled.data_ptr(), dx.data_ptr(), *geom(case), _st())
    splits = K.gemm_tn_splits(Out, In, N)
    slab = torch.empty(splits * Out * In, dtype=torch.float32, device="cuda")
    bslab = torch.empty(splits * Out, dtype=torch.float32, device="cuda")
    K.gemm_tn(d["dl"].data_ptr(), d["pooled"].data_ptr(), slab.data_ptr(), bslab.data_ptr(), Out, In, N, PLAIN,
              0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 0, 0, In, splits, _st())
    return (taken(dx, N * H * W * In, (N, H * W, In)),) + _reduced(K, slab, bslab, splits, In, Out)


def _dev(r):
    return {k: v.cuda() for k, v in r.items() if k in ("x", "w", "b", "dl", "pooled")}


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_head_fwd(K, case):
    assert K.head_supported(*geom(case), case[3])
    r = reference(case)
    d = _dev(r)
    pf, lf = run_fwd_fused(K, case, d)
    pu, lu = run_fwd_separate(K, case, d)
    check("pooled", pf, pu, r["pooled"], 2.0 ** -8)
    check("logits", lf, lu, r["logits"], 2.0 ** -8)
    pf2, lf2 = run_fwd_fused(K, case, d)
    assert torch.equal(pf, pf2) and torch.equal(lf, lf2)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_head_bwd(K, case):
    r = reference(case)
    d = _dev(r)
    xf, wf, bf = run_bwd_fused(K, case, d)
    xu, wu, bu = run_bwd_separate(K, case, d)
    check("dx", xf, xu, r["dx"], 2.0 ** -8)
    check("dW", wf, wu, r["dw"], 1e-6)
    check("db", bf, bu, r["db"], 1e-6)
    xf2, wf2, bf2 = run_bwd_fused(K, case, d)
    assert torch.equal(xf, xf2) and torch.equal(wf, wf2) and torch.equal(bf, bf2)


def test_head_bwd_without_input_gradient(K):
    """dx null: only the weight blocks run, with the same result."""
    case = CASES[2]
    N, (H, W), In, Out = case
    d = _dev(reference(case))
    _, wf, bf = run_bwd_fused(K, case, d)
    splits = K.head_bwd_splits(N, In, Out)
    slab, bslab = buf(splits * Out * In, torch.float32), buf(splits * Out, torch.float32)
    K.head_bwd(d["dl"].data_ptr(), d["w"].data_ptr(), d["pooled"].data_ptr(), 0, slab.data_ptr(), bslab.data_ptr(),
               *geom(case), Out, _st())
    w2, b2 = _reduced(K, slab, bslab, splits, In, Out)
    assert torch.equal(wf, w2) and torch.equal(bf, b2)


@pytest.mark.parametrize("g,out", [
    ((4, 4, 4, 96, 1, 1, 4, 4, 1, 1, 0, 0), 10),      # In = 96: not a multiple of 64
    ((4, 4, 4, 64, 3, 3, 2, 2, 1, 1, 0, 0), 10),      # a 2 x 2 window on a 4 x 4 map
    ((4, 1, 1, 4096, 1, 1, 1, 1, 1, 1, 0, 0), 10),    # In = 4096: past the LDS tile
], ids=["in96", "window2x2", "in4096"])
def test_head_unsupported_shapes_are_refused(K, g, out):
    assert not K.head_supported(*g, out)
    t = torch.zeros(1 << 16, dtype=BF16, device="cuda")
    f = torch.zeros(1 << 16, dtype=torch.float32, device="cuda")
    with pytest.raises((ValueError, RuntimeError)):
        K.head_fwd(t.data_ptr(), t.data_ptr(), 0, t.data_ptr(), t.data_ptr(), *g, out, _st())
    with pytest.raises((ValueError, RuntimeError)):
        K.head_bwd(t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), f.data_ptr(), f.data_ptr(), *g, out, _st())
