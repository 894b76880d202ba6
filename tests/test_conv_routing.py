"""Conv algorithm routing rules of ops/hip.py (`_hconv_ok`), checked on the CPU with the kernel
library's shape query stubbed: which convs go to the halo kernel (hconv / hconv3) instead of the
gathered GEMM or the streaming 1x1 kernel."""
import pytest

from dcnn_amd.ops import fusion, hip


class _Stub:
    def hconv_supported(self, *args):
        return True


@pytest.fixture
def stub(monkeypatch):
    monkeypatch.setattr(hip, "kernels", lambda: _Stub())
    monkeypatch.setattr(fusion, "HCONV_1X1", True)


TAP1 = [(0, 0, 0, 0)]
TAPS9 = [(dy, dx, 0, 0) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]


def test_3x3_same_stride1(stub):
    assert hip._hconv_ok(256, 32, 32, 32, 32, 1, 1, 64, 64, TAPS9, None)
    assert not hip._hconv_ok(256, 16, 16, 32, 32, 2, 2, 64, 128, TAPS9, None)  # strided
    # a tap two pixels away (5x5 reach) or more than 9 taps: not a halo-1 conv
    assert not hip._hconv_ok(256, 32, 32, 32, 32, 1, 1, 64, 64, [(2, 0, 0, 0), (0, 0, 0, 0)], None)
    assert not hip._hconv_ok(256, 32, 32, 32, 32, 1, 1, 64, 64, TAPS9 + [(0, 0, 0, 0)], None)


def test_1x1_only_k1024_small_grid(stub):
    # ResNet-50 batch 32: layer-3 reduce (1024 -> 256 at 8x8: 128 GEMM tiles) -> halo kernel
    assert hip._hconv_ok(32, 8, 8, 8, 8, 1, 1, 1024, 256, TAP1, None)
    assert hip._hconv_ok(32, 4, 4, 4, 4, 1, 1, 2048, 512, TAP1, None)
    # batch 256: 1024 tiles, the GEMM grid fills the chip
    assert not hip._hconv_ok(256, 8, 8, 8, 8, 1, 1, 1024, 256, TAP1, None)
    # K <= 512 1x1 convs belong to the streaming kernel / plain GEMM
    assert not hip._hconv_ok(32, 8, 8, 8, 8, 1, 1, 512, 256, TAP1, None)


def test_1x1_switch_off(stub, monkeypatch):
    monkeypatch.setattr(fusion, "HCONV_1X1", False)
    assert not hip._hconv_ok(32, 8, 8, 8, 8, 1, 1, 1024, 256, TAP1, None)


def test_1x1_split3_concat_stays_exact(stub):
    # fp32 concat callers pass Cs = 3 x Ci: a 384-channel fp32 1x1 conv (Cs = 1152) must not
    # leave the exact fp32 GEMM for the 3 x bf16 halo kernel (the K >= 1024 rule is bf16-only)
    assert not hip._hconv_ok(32, 8, 8, 8, 8, 1, 1, 3 * 384, 256, TAP1, None, True)
    assert not hip._hconv_ok(32, 4, 4, 4, 4, 1, 1, 3 * 2048, 512, TAP1, None, True)
    # 3x3 convs still take the split-precision halo path
    assert hip._hconv_ok(256, 32, 32, 32, 32, 1, 1, 3 * 64, 64, TAPS9, None, True)


def test_shared_route_table():
    """The kernel library's routing table (csrc/kernels/conv_route.cpp), which both the Python
    front end and the C++ host API's GPU backend ask: ResNet layer shapes land on the intended
    kernel families (host-side query, no GPU needed)."""
    from dcnn_amd.ops._ext import kernels
    K = kernels()

    def fwd(N, C, H, W, Co, k, s, p, mode=0):
        OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        return K.conv_fwd_route(N, C, H, W, Co, k, k, s, s, p, p, OH, OW, mode)

    assert fwd(256, 64, 32, 32, 64, 3, 1, 1) == K.ROUTE_HALO          # layer-1 3x3
    assert fwd(256, 256, 8, 8, 256, 3, 1, 1) == K.ROUTE_HALO          # 8x8 maps (gutter layout)
    assert fwd(256, 128, 16, 16, 256, 3, 2, 1) == K.ROUTE_GEMM_G2     # strided 3x3
    assert fwd(256, 64, 32, 32, 128, 1, 2, 0) == K.ROUTE_G1S          # strided 1x1 projection
    # K >= 1024 1x1, small grid: gemm_g2 split-K (default), the halo kernel's split-K without it
    prev = K.gemm_g2_splitk_enabled()
    try:
        K.gemm_g2_set_splitk(1)
        assert fwd(32, 1024, 8, 8, 256, 1, 1, 0) == K.ROUTE_GEMM_G2
        assert K.conv_dgrad_route(32, 256, 8, 8, 1024, 1, 1, 1, 1, 0, 0, 8, 8, 0) == K.ROUTE_GEMM_G2
        K.gemm_g2_set_splitk(0)
        assert fwd(32, 1024, 8, 8, 256, 1, 1, 0) == K.ROUTE_HALO
    finally:
        K.gemm_g2_set_splitk(prev)
    assert fwd(256, 1024, 8, 8, 256, 1, 1, 0) == K.ROUTE_GEMM_G2      # ... large grid
    assert fwd(8, 3, 32, 32, 16, 3, 1, 1) == K.ROUTE_GENERIC          # odd channel count
    assert fwd(256, 64, 32, 32, 256, 1, 1, 0, -1) != K.ROUTE_G1S      # epilogue not on g1s
    assert K.conv_dgrad_route(256, 64, 32, 32, 64, 3, 3, 1, 1, 1, 1, 32, 32, 2) == K.ROUTE_HALO
    assert K.conv_dgrad_route(256, 64, 32, 32, 256, 1, 1, 1, 1, 0, 0, 32, 32, 0) == K.ROUTE_G1S
    assert K.conv_wgrad_route(256, 64, 32, 32, 64, 3, 3, 1, 1, 1, 1, 32, 32, -1) == K.ROUTE_HALO
    assert K.conv_wgrad_route(256, 64, 32, 32, 128, 3, 3, 2, 2, 1, 1, 16, 16, -1) == K.ROUTE_HALO_S2  # stride-2 halo
    assert K.conv_wgrad_route(256, 64, 32, 32, 128, 1, 1, 2, 2, 0, 0, 16, 16, -1) == K.ROUTE_GEMM_G2  # strided 1x1


# (H, W, KH, KW, SH, SW, PH, PW)
TABLE_GEOMS = [
    (6, 6, 3, 3, 1, 1, 1, 1),      # plain 3x3 stride 1
    (8, 8, 3, 3, 2, 2, 1, 1),      # stride 2, four non-empty uniform phases
    (9, 7, 3, 3, 2, 2, 1, 1),      # non-uniform phases
    (8, 8, 1, 1, 2, 2, 0, 0),      # three empty phases
    (9, 9, 1, 1, 3, 3, 0, 0),      # nine phases, eight empty
    (8, 8, 2, 2, 2, 2, 0, 0),      # one tap per phase
    (8, 8, 5, 5, 2, 2, 2, 2),      # 5x5 stride 2
    (10, 10, 7, 7, 2, 2, 3, 3),    # 49 taps
    (6, 8, 1, 3, 1, 1, 0, 1),      # non-square kernel
    (8, 8, 3, 3, 2, 1, 1, 1),      # unequal strides
]


@pytest.mark.parametrize("geom", TABLE_GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_shared_tap_tables_exact(geom):
    """The shared tap tables (csrc/kernels/conv_args.cpp) reproduce the convolution exactly: the
    forward gathered with the forward table, the data gradient phase by phase with the phase list
    and the weight gradient with its table equal PyTorch's on integer-valued float64 tensors
    (NHWC rows, weights [Co][T][Ci], transposed weights [Ci][T][Co], as the kernels read them)."""
    import torch
    from dcnn_amd.ops._ext import kernels
    K = kernels()
    H, W, KH, KW, SH, SW, PH, PW = geom
    Ci, Co = 2, 3
    OH, OW = (H + 2 * PH - KH) // SH + 1, (W + 2 * PW - KW) // SW + 1
    gen = torch.Generator().manual_seed(sum(geom))
    x = torch.randint(-3, 4, (1, Ci, H, W), generator=gen).double()
    w = torch.randint(-3, 4, (Co, Ci, KH, KW), generator=gen).double()
    dy = torch.randint(-3, 4, (1, Co, OH, OW), generator=gen).double()
    x_hw, dy_hw = x[0].permute(1, 2, 0), dy[0].permute(1, 2, 0)
    xf, dyf = x_hw.reshape(-1), dy_hw.reshape(-1)
    wf = w.permute(0, 2, 3, 1).reshape(Co, -1)
    wtf = w.permute(1, 2, 3, 0).reshape(Ci, -1)

    def grid(h, w_):
        return torch.meshgrid(torch.arange(h), torch.arange(w_), indexing="ij")

    # forward: output pixel (oy, ox) reads the rows at its base + the tap's source offset
    oy, ox = grid(OH, OW)
    y = torch.zeros(OH, OW, Co, dtype=torch.float64)
    for tdy, tdx, src, b in K.conv_fwd_taps(Ci, W, KH, KW, PH, PW):
        iy, ix = oy * SH + tdy, ox * SW + tdx
        ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
        rows = xf[((oy * SH * W + ox * SW) * Ci + src)[ok][:, None] + torch.arange(Ci)]
        y[ok] += rows @ wf[:, b:b + Ci].T
    assert torch.equal(y.permute(2, 0, 1)[None], torch.nn.functional.conv2d(x, w, stride=(SH, SW), padding=(PH, PW)))

    # data gradient: phase (ry, rx) is a dense GH x GW conv of dy over its own taps
    phases, taps = K.conv_dgrad_phases(H, W, OW, Co, KH, KW, SH, SW, PH, PW)
    dx = torch.full((H, W, Ci), float("nan"), dtype=torch.float64)
    for ry, rx, GH, GW, t0, nt in phases:
        gy, gx = grid(GH, GW)
        acc = torch.zeros(GH, GW, Ci, dtype=torch.float64)
        for tdy, tdx, src, b in taps[t0:t0 + nt]:
            sy, sx = gy + tdy, gx + tdx
            ok = (sy >= 0) & (sy < OH) & (sx >= 0) & (sx < OW)
            rows = dyf[((gy * OW + gx) * Co + src)[ok][:, None] + torch.arange(Co)]
            acc[ok] += rows @ wtf[:, b:b + Co].T
        assert torch.isnan(dx[ry::SH, rx::SW]).all()  # every input pixel belongs to one phase
        dx[ry::SH, rx::SW] = acc
    assert torch.equal(dx.permute(2, 0, 1)[None],
                       torch.nn.grad.conv2d_input(x.shape, w, dy, stride=(SH, SW), padding=(PH, PW)))

    # weight gradient: tap t pairs dy at (oy, ox) with x at (oy SH + dy_t, ox SW + dx_t)
    dw = torch.zeros(Co, KH * KW, Ci, dtype=torch.float64)
    for t, (tdy, tdx) in enumerate(K.conv_wgrad_taps(KH, KW, PH, PW)):
        iy, ix = oy * SH + tdy, ox * SW + tdx
        ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
        dw[:, t] = dy_hw[ok].T @ x_hw[iy[ok], ix[ok]]
    assert torch.equal(dw.reshape(Co, KH, KW, Ci).permute(0, 3, 1, 2),
                       torch.nn.grad.conv2d_weight(x, w.shape, dy, stride=(SH, SW), padding=(PH, PW)))


@pytest.mark.parametrize("geom", TABLE_GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_shared_dgrad_phase_list_structure(geom):
    """One entry per stride phase with GH, GW > 0, in (ry, rx) order, zero-tap phases included;
    the phases' tap ranges tile the flat table."""
    from dcnn_amd.ops._ext import kernels
    H, W, KH, KW, SH, SW, PH, PW = geom
    OW = (W + 2 * PW - KW) // SW + 1
    phases, taps = kernels().conv_dgrad_phases(H, W, OW, 3, KH, KW, SH, SW, PH, PW)
    want = [(ry, rx, len(range(ry, H, SH)), len(range(rx, W, SW))) for ry in range(SH) for rx in range(SW)
            if ry < H and rx < W]
    assert [tuple(p[:4]) for p in phases] == want
    t = 0
    for p in phases:
        assert p[4] == t and p[5] >= 0
        t += p[5]
    assert t == len(taps) == sum(p[5] for p in phases)
