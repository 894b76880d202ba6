"""Grouped convolution (1 < groups < C) on the MFMA HIP kernels of gconv.hip: NHWC activations (bf16,
or fp32 for the fp32 compute mode), weights ``(Co, Ci/G, KH, KW)`` channels_last in the activation
dtype, fp32 bias and gradients. No reference counterpart (the reference has no grouped
convolution); semantics are ``F.conv2d(groups=G)``."""
from __future__ import annotations

from ._ext import dt_code, kernels, ptr, stream_ptr
from .hip_base import CL, F32, _check_act, _empty, _rec, _reduce_wb, conv_out_hw

_SIZES = "{4, 8, 16} or a multiple of 32"


def _gc_geom(what, N, Ci, Co, G, H, W, KH, KW, stride, pad):
    if G < 1 or Ci % G or Co % G:
        raise ValueError(f"{what}: unsupported grouped conv: Ci={Ci}, Co={Co} not divisible by groups G={G}")
    OH, OW = conv_out_hw(H, W, KH, KW, stride[0], stride[1], pad[0], pad[1])
    return [N, H, W, Ci, Co, G, OH, OW, KH, KW, stride[0], stride[1], pad[0], pad[1]]


def _gc_check(K, what, dtype, g):
    """A shape the kernels do not take is an error naming the shape (never a fallback)."""
    N, H, W, Ci, Co, G, OH, OW, KH, KW, SH, SW, PH, PW = g
    if OH < 1 or OW < 1 or not K.gconv_supported(dt_code(dtype), g):
        raise ValueError(f"{what}: unsupported grouped conv: x (N={N}, Ci={Ci}, H={H}, W={W}) {dtype}, Co={Co}, "
                         f"G={G} (Cig={Ci // G}, Cog={Co // G}), kernel {KH}x{KW}, stride {SH}x{SW}, pad {PH}x{PW} "
                         f"(needs G >= 2, Cig and Cog each in {_SIZES}, KH*KW <= 49, pad < kernel, fewer than "
                         f"2^31 elements)")


def _gc_weight(w, Co, Cig, KH, KW, dtype, what):
    if tuple(w.shape) != (Co, Cig, KH, KW) or w.dtype != dtype:
        raise ValueError(f"{what}: weights {tuple(w.shape)} {w.dtype}, expected {(Co, Cig, KH, KW)} {dtype}")
    if not w.is_contiguous(memory_format=CL):
        raise ValueError(f"{what}: weights must be channels_last ([Co][KH][KW][Cig])")
    return w


def gconv_wgrad_splits(dy_dtype, x_shape, w_shape, stride, pad, groups):
    """Split count :func:`gconv2d_wgrad` uses for this shape (slab rows)."""
    N, Ci, H, W = x_shape
    K = kernels()
    g = _gc_geom("gconv_wgrad_splits", N, Ci, w_shape[0], groups, H, W, w_shape[2], w_shape[3], stride, pad)
    _gc_check(K, "gconv_wgrad_splits", dy_dtype, g)
    return K.gconv_wgrad_splits(dt_code(dy_dtype), g)


def gconv2d_fwd(x, w, bias, stride, pad, groups):
    """y = conv(x, w, groups) + bias. x: (N,Ci,H,W) channels_last bf16 / fp32, w: (Co,Ci/G,KH,KW)
    channels_last of x's dtype, bias: fp32 [Co] or None. fp32 accumulation, one rounding at the store."""
    _check_act(x, "gconv2d_fwd.x")
    K = kernels()
    N, Ci, H, W = x.shape
    Co, KH, KW = w.shape[0], w.shape[2], w.shape[3]
    g = _gc_geom("gconv2d_fwd", N, Ci, Co, groups, H, W, KH, KW, stride, pad)
    _gc_check(K, "gconv2d_fwd", x.dtype, g)
    _gc_weight(w, Co, Ci // groups, KH, KW, x.dtype, "gconv2d_fwd")
    _rec("gc_fwd", x=(N, Ci, H, W), w=(Co, Ci // groups, KH, KW), groups=groups, stride=tuple(stride),
         pad=tuple(pad), bias=bias is not None)
    if bias is not None:
        assert bias.dtype == F32 and bias.numel() == Co and bias.is_contiguous()
    y = _empty((N, Co, g[6], g[7]), x.dtype, x.device, True)
    K.gconv_fwd(dt_code(x.dtype), x.data_ptr(), w.data_ptr(), ptr(bias), y.data_ptr(), g, stream_ptr())
    return y


def gconv2d_dgrad(dy, w, x_shape, stride, pad, groups, *, residual=None):
    """dx = conv^T(dy, w, groups) (+ residual, a channels_last activation of x's shape); gather form:
    input positions no output reaches get 0 (+ residual). The [Ci][KH][KW][Co/G] operand is made from
    w by one small transpose launch."""
    _check_act(dy, "gconv2d_dgrad.dy")
    K = kernels()
    N, Ci, H, W = x_shape
    Co, KH, KW = w.shape[0], w.shape[2], w.shape[3]
    g = _gc_geom("gconv2d_dgrad", N, Ci, Co, groups, H, W, KH, KW, stride, pad)
    _gc_check(K, "gconv2d_dgrad", dy.dtype, g)
    _gc_weight(w, Co, Ci // groups, KH, KW, dy.dtype, "gconv2d_dgrad")
    if tuple(dy.shape) != (N, Co, g[6], g[7]):
        raise ValueError(f"gconv2d_dgrad: dy {tuple(dy.shape)}, expected {(N, Co, g[6], g[7])}")
    _rec("gc_dgrad", x=(N, Ci, H, W), w=(Co, Ci // groups, KH, KW), groups=groups, stride=tuple(stride),
         pad=tuple(pad), residual=residual is not None)
    if residual is not None:
        assert tuple(residual.shape) == (N, Ci, H, W) and residual.dtype == dy.dtype
        assert residual.is_contiguous(memory_format=CL)
    dt, st = dt_code(dy.dtype), stream_ptr()
    wt = _empty((Ci * KH * KW * (Co // groups),), dy.dtype, dy.device)
    K.gconv_weight_t(dt, w.data_ptr(), wt.data_ptr(), g, st)
    dx = _empty((N, Ci, H, W), dy.dtype, dy.device, True)
    K.gconv_dgrad(dt, dy.data_ptr(), wt.data_ptr(), ptr(residual), dx.data_ptr(), g, st)
    return dx


def gconv2d_wgrad(dy, x, w_shape, stride, pad, groups, grad_w, grad_b=None):
    """grad_w += dW (fp32, (Co,Ci/G,KH,KW) channels_last), grad_b += sum(dy) over (N, OH, OW):
    per-split partial slabs summed in a fixed order (bit-reproducible)."""
    _check_act(dy, "gconv2d_wgrad.dy")
    _check_act(x, "gconv2d_wgrad.x")
    K = kernels()
    N, Ci, H, W = x.shape
    Co, Cig, KH, KW = w_shape
    g = _gc_geom("gconv2d_wgrad", N, Ci, Co, groups, H, W, KH, KW, stride, pad)
    _gc_check(K, "gconv2d_wgrad", x.dtype, g)
    if Cig != Ci // groups or tuple(dy.shape) != (N, Co, g[6], g[7]) or dy.dtype != x.dtype:
        raise ValueError(f"gconv2d_wgrad: dy {tuple(dy.shape)} {dy.dtype}, x {tuple(x.shape)} {x.dtype}, "
                         f"w {tuple(w_shape)}, groups {groups}")
    n = Co * KH * KW * Cig
    assert grad_w.dtype == F32 and grad_w.numel() == n
    assert grad_w.is_contiguous(memory_format=CL), "channels_last fp32 weight gradient ([Co][KH][KW][Cig])"
    _rec("gc_wgrad", x=(N, Ci, H, W), w=(Co, Cig, KH, KW), groups=groups, stride=tuple(stride), pad=tuple(pad),
         bias=grad_b is not None)
    dt = dt_code(x.dtype)
    splits = K.gconv_wgrad_splits(dt, g)
    slab = _empty((splits, n), F32, x.device)
    bslab = _empty((splits, Co), F32, x.device) if grad_b is not None else None
    st = stream_ptr()
    K.gconv_wgrad(dt, dy.data_ptr(), x.data_ptr(), slab.data_ptr(), ptr(bslab), g, st)
    _reduce_wb(K, slab, grad_w, n, bslab, grad_b, Co, splits, st)
