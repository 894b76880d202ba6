"""Depthwise convolution (groups = C, channel multiplier 1) on the streaming HIP kernels of
dwconv.hip: NHWC activations (bf16, or fp32 for the fp32 compute mode), weights ``(C,1,KH,KW)`` in
the activation dtype, fp32 bias and gradients. No reference counterpart (the reference has no
grouped convolution); semantics are ``F.conv2d(groups=C)``."""
from __future__ import annotations

from ._ext import dt_code, kernels, ptr, stream_ptr
from .hip_base import CL, F32, _check_act, _empty, _rec, _reduce_wb, conv_out_hw


def _dw_geom(N, C, H, W, KH, KW, stride, pad):
    OH, OW = conv_out_hw(H, W, KH, KW, stride[0], stride[1], pad[0], pad[1])
    return [N, H, W, C, OH, OW, KH, KW, stride[0], stride[1], pad[0], pad[1]]


def _dw_check(K, what, dtype, g):
    """A shape the kernels do not take is an error naming the shape (never a fallback)."""
    N, H, W, C, OH, OW, KH, KW, SH, SW, PH, PW = g
    if OH < 1 or OW < 1 or not K.dwconv_supported(dt_code(dtype), g):
        raise ValueError(f"{what}: unsupported depthwise conv: x (N={N}, C={C}, H={H}, W={W}) {dtype}, kernel "
                         f"{KH}x{KW}, stride {SH}x{SW}, pad {PH}x{PW} (needs C % {4 if dtype == F32 else 8} == 0, "
                         f"KH*KW <= 49, pad < kernel, fewer than 2^31 elements)")


def _dw_weight(w, C, KH, KW, dtype, what):
    if tuple(w.shape) != (C, 1, KH, KW) or w.dtype != dtype:
        raise ValueError(f"{what}: weights {tuple(w.shape)} {w.dtype}, expected {(C, 1, KH, KW)} {dtype}")
    # one input channel per filter: NCHW-contiguous and channels_last are the same bytes [C][KH][KW]
    assert w.is_contiguous() or w.is_contiguous(memory_format=CL)
    return w


def dwconv_wgrad_splits(dy_dtype, x_shape, w_shape, stride, pad):
    """Split count :func:`dwconv2d_wgrad` uses for this shape (slab rows)."""
    N, C, H, W = x_shape
    return kernels().dwconv_wgrad_splits(dt_code(dy_dtype), _dw_geom(N, C, H, W, w_shape[2], w_shape[3], stride, pad))


def dwconv2d_fwd(x, w, bias, stride, pad):
    """y = depthwise_conv(x, w) + bias. x: (N,C,H,W) channels_last bf16 / fp32, w: (C,1,KH,KW) of
    x's dtype, bias: fp32 [C] or None. fp32 accumulation, one rounding at the store."""
    _check_act(x, "dwconv2d_fwd.x")
    K = kernels()
    N, C, H, W = x.shape
    KH, KW = w.shape[2], w.shape[3]
    g = _dw_geom(N, C, H, W, KH, KW, stride, pad)
    _dw_check(K, "dwconv2d_fwd", x.dtype, g)
    _dw_weight(w, C, KH, KW, x.dtype, "dwconv2d_fwd")
    _rec("dw_fwd", x=(N, C, H, W), w=(C, 1, KH, KW), stride=tuple(stride), pad=tuple(pad), bias=bias is not None)
    if bias is not None:
        assert bias.dtype == F32 and bias.numel() == C and bias.is_contiguous()
    y = _empty((N, C, g[4], g[5]), x.dtype, x.device, True)
    K.dwconv_fwd(dt_code(x.dtype), x.data_ptr(), w.data_ptr(), ptr(bias), y.data_ptr(), g, stream_ptr())
    return y


def dwconv2d_dgrad(dy, w, x_shape, stride, pad, *, residual=None):
    """dx = depthwise_conv^T(dy, w) (+ residual, a channels_last activation of x's shape); gather
    form: input positions no output reaches get 0 (+ residual)."""
    _check_act(dy, "dwconv2d_dgrad.dy")
    K = kernels()
    N, C, H, W = x_shape
    KH, KW = w.shape[2], w.shape[3]
    g = _dw_geom(N, C, H, W, KH, KW, stride, pad)
    _dw_check(K, "dwconv2d_dgrad", dy.dtype, g)
    _dw_weight(w, C, KH, KW, dy.dtype, "dwconv2d_dgrad")
    if tuple(dy.shape) != (N, C, g[4], g[5]):
        raise ValueError(f"dwconv2d_dgrad: dy {tuple(dy.shape)}, expected {(N, C, g[4], g[5])}")
    _rec("dw_dgrad", x=(N, C, H, W), w=(C, 1, KH, KW), stride=tuple(stride), pad=tuple(pad),
         residual=residual is not None)
    if residual is not None:
        assert tuple(residual.shape) == (N, C, H, W) and residual.dtype == dy.dtype
        assert residual.is_contiguous(memory_format=CL)
    dx = _empty((N, C, H, W), dy.dtype, dy.device, True)
    K.dwconv_dgrad(dt_code(dy.dtype), dy.data_ptr(), w.data_ptr(), ptr(residual), dx.data_ptr(), g, stream_ptr())
    return dx


def dwconv2d_wgrad(dy, x, w_shape, stride, pad, grad_w, grad_b=None):
    """grad_w += dW (fp32, (C,1,KH,KW)), grad_b += sum(dy) over (N, OH, OW): per-split partial
    slabs summed in a fixed order (bit-reproducible)."""
    _check_act(dy, "dwconv2d_wgrad.dy")
    _check_act(x, "dwconv2d_wgrad.x")
    K = kernels()
    N, C, H, W = x.shape
    KH, KW = w_shape[2], w_shape[3]
    g = _dw_geom(N, C, H, W, KH, KW, stride, pad)
    _dw_check(K, "dwconv2d_wgrad", x.dtype, g)
    if tuple(w_shape) != (C, 1, KH, KW) or tuple(dy.shape) != (N, C, g[4], g[5]) or dy.dtype != x.dtype:
        raise ValueError(f"dwconv2d_wgrad: dy {tuple(dy.shape)} {dy.dtype}, x {tuple(x.shape)} {x.dtype}, "
                         f"w {tuple(w_shape)}")
    assert grad_w.dtype == F32 and grad_w.numel() == C * KH * KW
    assert grad_w.is_contiguous() or grad_w.is_contiguous(memory_format=CL), "dense fp32 weight gradient"
    _rec("dw_wgrad", x=(N, C, H, W), w=(C, 1, KH, KW), stride=tuple(stride), pad=tuple(pad), bias=grad_b is not None)
    dt = dt_code(x.dtype)
    splits = K.dwconv_wgrad_splits(dt, g)
    n = C * KH * KW
    slab = _empty((splits, n), F32, x.device)
    bslab = _empty((splits, C), F32, x.device) if grad_b is not None else None
    st = stream_ptr()
    K.dwconv_wgrad(dt, dy.data_ptr(), x.data_ptr(), slab.data_ptr(), ptr(bslab), g, st)
    _reduce_wb(K, slab, grad_w, n, bslab, grad_b, C, splits, st)
