"""A downsample block's shortcut gradient kept phase-compact (DCNN_COMPACT_SHORTCUT_GRAD).

A 1x1 stride-2 pad-0 shortcut conv's data gradient only reaches the even pixels. The C++ engine
keeps it as the [N, H/2, W/2, Ci] tensor of those pixels (gpu_ops::conv_dgrad_compact) and the
head conv's stride-phase-grouped gemm_g2 data gradient adds it in its phase (0, 0) class alone
(G2Args::res_cls), instead of writing a full-size tensor three quarters zero and reading it back
in every phase. No arithmetic changes, so every comparison here is bit for bit:

* kernel level (C ABI of libdcnn.so): the 3x3 stride-2 pad-1 data gradient with a compact residual
  against the same call with the full-size residual (the compact values at the even pixels, zeros
  elsewhere): dx, and the fused BatchNorm backward's statistics rows, identical bits; relative L2
  against an fp64 reference no larger than the full-size path's (printed); sentinel tails behind dx
  (must stay) and behind the compact tensor (NaN: a read past its end would poison dx); every case
  run twice. Inputs hold products that underflow to -0.0 (printed: how many -0.0 the plain data
  gradient stores), which both paths turn into +0.0 by the residual add;
* invalid uses raise: a compact residual on a stride-1 conv, on a conv whose phase (0, 0) no tap
  reaches, and gemm_g2 itself on a res_cls out of range, naming an empty class, or ungrouped;
* the compact projection gradient equals the even-pixel entries of the full-size one, whose other
  entries are zero;
* block level: one downsample ResidualBlock (64 -> 128, 16x16, N = 8) of the C++ engine with the
  switch on and off: dx and every parameter gradient identical bits, and the recorded conv calls
  show the compact pair ran only with the switch on.
"""
import ctypes
import json
import os
import subprocess

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "dcnn_amd", "libdcnn.so")
PARITY = os.path.join(ROOT, "dcnn_amd", "bin", "host_api_parity")
P = ctypes.c_void_p
BF = torch.bfloat16
TAIL = 4096  # sentinel elements behind a buffer

# (N, H, W, Ci, Co, fused BatchNorm backward)
CASES = [(2, 16, 16, 64, 128, False), (8, 8, 8, 128, 256, False), (4, 16, 16, 256, 512, False),
         (2, 32, 32, 64, 64, False), (2, 16, 16, 64, 128, True)]


@pytest.fixture(scope="module")
def L():
    if not (os.path.exists(LIB) and os.path.exists(PARITY)):
        from dcnn_amd import _build
        _build.build_host()
    lib = ctypes.CDLL(LIB)
    lib.dcnn_c_last_error.restype = ctypes.c_char_p
    for name in ("dcnn_c_conv_dgrad", "dcnn_c_conv_dgrad_compact_residual", "dcnn_c_conv_dgrad_compact",
                 "dcnn_c_conv_dgrad_takes_compact", "dcnn_c_copy"):
        getattr(lib, name).restype = ctypes.c_int
    return lib


def _ok(L, rc):
    assert rc == 0, L.dcnn_c_last_error().decode()


def _ptr(t):
    return P(t.data_ptr() if t is not None else 0)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def _tailed(n, fill_bits):
    """bf16 buffer of n elements + TAIL sentinel elements (bit pattern fill_bits)."""
    buf = torch.empty(n + TAIL, dtype=torch.int16, device="cuda")
    buf.fill_(fill_bits)
    return buf.view(BF)


def _shape(N, Ci, H, W, Co, k, s, p):
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    return (ctypes.c_int * 13)(N, Ci, H, W, Co, k, k, s, s, p, p, OH, OW), OH, OW


_INPUTS = {}


def _inputs(case):
    """Operands of one case (NHWC memory) and the fp64 reference, computed once and left unchanged."""
    if case in _INPUTS:
        return _INPUTS[case]
    N, H, W, Ci, Co, bnb = case
    g = torch.Generator().manual_seed(1000 + N + H + Ci + Co)
    OH, OW = H // 2, W // 2
    dy = torch.randn(N, OH, OW, Co, generator=g)
    w = torch.randn(Co, 3, 3, Ci, generator=g) * (2.0 / (9 * Ci)) ** 0.5
    # image 0: products that underflow (negative): -2^-130 / -2^-140 / -2^-150 each, on three input
    # channels; an accumulator of those rounds to a bf16 -0.0 (or a negative denormal)
    dy[0] = -(2.0 ** -70)
    w[:, :, :, 0] = 2.0 ** -60
    w[:, :, :, 1] = 2.0 ** -70
    w[:, :, :, 2] = 2.0 ** -80
    resc = torch.randn(N, OH, OW, Ci, generator=g)
    resc[:, :, :, 0:3] = 0.0      # the residual leaves the underflowing channels alone ...
    resc[0, :, :, 1] = -0.0       # ... or adds -0.0
    resc[1, 0, :, :] = 0.0
    dy, w, resc = dy.to(BF), w.to(BF), resc.to(BF)
    ops = {"dy": dy.cuda(), "w": w.cuda()}
    rc = _tailed(resc.numel(), 0x7FC0)  # NaN behind the compact tensor
    rc[:resc.numel()] = resc.cuda().reshape(-1)
    ops["resc_buf"] = rc
    full = torch.zeros(N, H, W, Ci, dtype=BF)
    full[:, ::2, ::2] = resc
    ops["resf"] = full.cuda()
    if bnb:
        xb = (torch.randn(N, H, W, Ci, generator=g) * 2 + 0.5).to(BF)
        mean = xb.float().mean((0, 1, 2)).contiguous()
        istd = torch.rsqrt(xb.float().var((0, 1, 2), unbiased=False) + 1e-5).contiguous()
        gam, bet = torch.randn(Ci, generator=g), torch.randn(Ci, generator=g)
        yb = ((xb.float() - mean) * (istd * gam) + bet).clamp_min(0).to(BF)
        ops.update(xb=xb.cuda(), yb=yb.cuda(), mean=mean.cuda(), istd=istd.cuda())
    # fp64 reference from the same bf16 operands (CPU)
    wd = w.double().permute(0, 3, 1, 2).contiguous()       # (Co, Ci, 3, 3)
    dyd = dy.double().permute(0, 3, 1, 2).contiguous()     # (N, Co, OH, OW)
    ref = torch.nn.grad.conv2d_input((N, Ci, H, W), wd, dyd, 2, 1).permute(0, 2, 3, 1) + full.double()
    if bnb:
        ref = ref * (ops["yb"].cpu().double() > 0)
    ops["ref"] = ref
    _INPUTS[case] = ops
    return ops


def _run(L, case, compact):
    """One data gradient -> (dx [N, H, W, Ci], statistics rows or None); checks dx's sentinel tail."""
    N, H, W, Ci, Co, bnb = case
    o = _inputs(case)
    shape, _, _ = _shape(N, Ci, H, W, Co, 3, 2, 1)
    n = N * H * W * Ci
    dxb = _tailed(n, 0x7F7F)
    slab, rows = ctypes.c_void_p(), ctypes.c_int(0)
    b = [int(bnb), _ptr(o.get("yb")), _ptr(o.get("xb")), _ptr(o.get("mean")), _ptr(o.get("istd")),
         ctypes.byref(slab), ctypes.byref(rows)]
    torch.cuda.synchronize()
    if compact:
        _ok(L, L.dcnn_c_conv_dgrad_compact_residual(_ptr(o["dy"]), _ptr(o["w"]), _ptr(dxb), shape,
                                                    _ptr(o["resc_buf"]), *b))
    else:
        _ok(L, L.dcnn_c_conv_dgrad(_ptr(o["dy"]), _ptr(o["w"]), 1, _ptr(dxb), shape, _ptr(o["resf"]), *b))
    st = None
    if bnb:
        assert rows.value > 0, "the fused BatchNorm backward was not honoured"
        st = torch.empty(rows.value, 2, Ci, device="cuda")
        _ok(L, L.dcnn_c_copy(_ptr(st), slab, ctypes.c_size_t(st.numel() * 4)))
    assert bool((_bits(dxb[n:]) == 0x7F7F).all()), "dx: the sentinel tail was written"
    return dxb[:n].view(N, H, W, Ci).clone(), st


def _rel(a, ref):
    return float((a.cpu().double() - ref).norm() / ref.norm().clamp_min(1e-300))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_compact_residual_equals_full_size_residual(L, case):
    N, H, W, Ci, Co, bnb = case
    shape, _, _ = _shape(N, Ci, H, W, Co, 3, 2, 1)
    assert L.dcnn_c_conv_dgrad_takes_compact(shape) == 1
    o = _inputs(case)
    full, st_f = _run(L, case, False)
    comp, st_c = _run(L, case, True)
    # how many -0.0 the epilogue is handed: the plain data gradient (no residual add) stores them
    if not bnb:
        plain = torch.empty(N, H, W, Ci, dtype=BF, device="cuda")
        _ok(L, L.dcnn_c_conv_dgrad(_ptr(o["dy"]), _ptr(o["w"]), 1, _ptr(plain), shape, P(0), 0, P(0), P(0), P(0), P(0),
                                   None, None))
        neg0 = int((_bits(plain) == -32768).sum())
        print(f"{case}: -0.0 stored by the plain data gradient: {neg0}; by the residual paths: "
              f"{int((_bits(full) == -32768).sum())} full, {int((_bits(comp) == -32768).sum())} compact")
    ef, ec = _rel(full, o["ref"]), _rel(comp, o["ref"])
    print(f"{case}: rel L2 vs fp64: full-size {ef:.6e}, compact {ec:.6e}")
    assert not bool(torch.isnan(comp.float()).any()), "compact: NaN (a read behind the compact tensor?)"
    assert torch.equal(_bits(comp), _bits(full)), int((_bits(comp) != _bits(full)).sum())
    assert ec <= ef and ef < 1e-2
    if bnb:
        assert torch.equal(_bits(st_c), _bits(st_f)), "fused BatchNorm backward statistics rows"
        assert bool((comp[o["yb"] <= 0] == 0).all())
    # twice: the same bits
    comp2, st_c2 = _run(L, case, True)
    assert torch.equal(_bits(comp2), _bits(comp))
    if bnb:
        assert torch.equal(_bits(st_c2), _bits(st_c))
    # the operands were only read
    n = N * (H // 2) * (W // 2) * Ci
    assert bool((_bits(o["resc_buf"][n:]) == 0x7FC0).all())


def test_compact_residual_invalid_uses_raise(L):
    N, H, W, Ci, Co = 2, 16, 16, 64, 128
    dy = torch.zeros(N * H * W * Co, dtype=BF, device="cuda")
    w = torch.zeros(Co * 9 * Ci, dtype=BF, device="cuda")
    dx = torch.zeros(N * H * W * Ci, dtype=BF, device="cuda")
    res = torch.zeros(N * H * W * Ci, dtype=BF, device="cuda")
    none = [0, P(0), P(0), P(0), P(0), None, None]
    # a stride-1 conv (the halo route), and a 1x1 stride-2 pad-1 conv (no tap reaches phase (0, 0))
    for k, s, p in ((3, 1, 1), (1, 2, 1)):
        shape, _, _ = _shape(N, Ci, H, W, Co, k, s, p)
        assert L.dcnn_c_conv_dgrad_takes_compact(shape) == 0
        rc = L.dcnn_c_conv_dgrad_compact_residual(_ptr(dy), _ptr(w), _ptr(dx), shape, _ptr(res), *none)
        assert rc == -1 and b"phase-compact" in L.dcnn_c_last_error()
    # no residual at all
    shape, _, _ = _shape(N, Ci, H, W, Co, 3, 2, 1)
    assert L.dcnn_c_conv_dgrad_compact_residual(_ptr(dy), _ptr(w), _ptr(dx), shape, P(0), *none) == -1
    # the compact projection gradient is a strided 1x1 pad-0 conv's
    assert L.dcnn_c_conv_dgrad_compact(_ptr(dy), _ptr(w), _ptr(dx), shape) == -1
    # gemm_g2 itself (raw binding): the 1x1 stride-2 data gradient's classes, three of them empty
    import dcnn_amd._kernels as K
    OH = OW = H // 2
    phases, taps = K.conv_dgrad_phases(H, W, OW, Co, 1, 1, 2, 2, 0, 0)
    groups = [(t0, nt, ry, rx) for ry, rx, GH, GW, t0, nt in phases]
    assert [g[1] for g in groups] == [1, 0, 0, 0]
    M = 4 * N * OH * OW

    def call(res_cls, groups=groups, m=M, residual=res.data_ptr()):
        K.gemm_g2_res_cls(0, dy.data_ptr(), w.data_ptr(), dx.data_ptr(), N * OH * OW * Co * 2, Ci * Co * 2, m, Ci, Co, OH,
                          OW, OH, OW, 1, 1, [tuple(t) for t in taps], Co, Ci, H, W, 2, 2, 0, 0, 0, residual, 0, 0, 0, 0,
                          (0, 0, 0, 0), 0, groups, res_cls)

    with pytest.raises(RuntimeError, match="without taps"):
        call(1)
    with pytest.raises(RuntimeError, match="out of range"):
        call(4)
    with pytest.raises(RuntimeError, match="grouped launch"):
        call(0, groups=[], m=N * OH * OW)
    with pytest.raises(RuntimeError, match="grouped launch"):
        call(0, residual=0)
    torch.cuda.synchronize()


@pytest.mark.parametrize("Ci,Co", [(64, 128), (128, 256), (256, 512)])
def test_compact_projection_gradient_equals_even_pixels(L, Ci, Co):
    N, H, W = 4, 16, 16
    g = torch.Generator().manual_seed(Ci)
    shape, OH, OW = _shape(N, Ci, H, W, Co, 1, 2, 0)
    dy = torch.randn(N, OH, OW, Co, generator=g).to(BF).cuda()
    dy[0, 0] = -(2.0 ** -70)
    w = (torch.randn(Co, Ci, generator=g) * (2.0 / Ci) ** 0.5)
    w[:, 0] = 2.0 ** -70
    w = w.to(BF).cuda()
    nf, nc = N * H * W * Ci, N * OH * OW * Ci
    fullb, compb = _tailed(nf, 0x7F7F), _tailed(nc, 0x7F7F)
    torch.cuda.synchronize()
    _ok(L, L.dcnn_c_conv_dgrad(_ptr(dy), _ptr(w), 1, _ptr(fullb), shape, P(0), 0, P(0), P(0), P(0), P(0), None, None))
    _ok(L, L.dcnn_c_conv_dgrad_compact(_ptr(dy), _ptr(w), _ptr(compb), shape))
    assert bool((_bits(fullb[nf:]) == 0x7F7F).all()) and bool((_bits(compb[nc:]) == 0x7F7F).all())
    full, comp = fullb[:nf].view(N, H, W, Ci), compb[:nc].view(N, OH, OW, Ci)
    assert torch.equal(_bits(comp), _bits(full[:, ::2, ::2]))
    off = full.clone()
    off[:, ::2, ::2] = 0
    assert bool((_bits(off) == 0).all()), "the full-size gradient off the even pixels"
    ref = (dy.cpu().double().reshape(-1, Co) @ w.cpu().double()).reshape(N, OH, OW, Ci)
    print(f"projection {Ci}/{Co}: rel L2 vs fp64 {_rel(comp, ref):.3e}, -0.0 entries {int((_bits(comp) == -32768).sum())}")
    assert _rel(comp, ref) < 1e-2
    # the routing table's choice for the same stride-1 GEMM (the streaming kernel where it applies):
    # reported only — the compact gradient stays on gemm_g2, the kernel and K order of the full-size one
    s1, _, _ = _shape(N, Ci, OH, OW, Co, 1, 1, 0)
    alt = torch.empty(N, OH, OW, Ci, dtype=BF, device="cuda")
    _ok(L, L.dcnn_c_conv_dgrad(_ptr(dy), _ptr(w), 1, _ptr(alt), s1, P(0), 0, P(0), P(0), P(0), P(0), None, None))
    print(f"projection {Ci}/{Co}: routed stride-1 data gradient differs from gemm_g2's in "
          f"{int((_bits(alt) != _bits(comp)).sum())} of {nc} entries")


def test_cpp_downsample_block_switch_bit_identical(L, tmp_path):
    from dcnn_amd.nn.sequential import load_tensor
    res = {}
    for on in ("1", "0"):
        rec = tmp_path / f"ops{on}.jsonl"
        env = dict(os.environ, DCNN_COMPACT_SHORTCUT_GRAD=on, DCNN_RECORD_OPS=str(rec))
        r = subprocess.run([PARITY, "resblock", "64", "128", "16", "8", f"g{on}.bin", "--device", "GPU"], cwd=tmp_path,
                           env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:]
        names = [l.split()[1:] for l in r.stdout.splitlines() if l.startswith("params")][0]
        with open(tmp_path / f"g{on}.bin", "rb") as f:
            grads = [load_tensor(f) for _ in names]
        with open(rec) as f:
            ops = [json.loads(l) for l in f if l.strip()]
        res[on] = (names, grads, [c for c in ops if c["op"] == "dgrad"])
    names, g1, d1 = res["1"]
    names0, g0, d0 = res["0"]
    assert names == names0 and names[0] == "dx" and len(names) == 12
    assert tuple(g1[0].shape) == (8, 64, 16, 16) and float(g1[0].abs().max()) > 0
    for n, a, b in zip(names, g1, g0):
        assert torch.equal(_bits(a), _bits(b)), (n, float((a - b).abs().max()))
    # the compact pair ran with the switch on only: a stride-1 projection gradient on dy's grid
    # and a head data gradient with the compact residual
    assert [c["residual_compact"] for c in d1 if c["residual"]] == [1]
    assert [c["residual_compact"] for c in d0 if c["residual"]] == [0]
    assert any(c["shape"][1:4] == [64, 8, 8] and c["shape"][7:9] == [1, 1] for c in d1)
    assert any(c["shape"][1:4] == [64, 16, 16] and c["shape"][5:9] == [1, 1, 2, 2] for c in d0)
    assert not any(c["shape"][5:9] == [1, 1, 2, 2] for c in d1)
