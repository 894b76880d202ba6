"""Native CPU backend (``_native.cpu``, csrc/native/cpu_ops.cpp + cpu_gemm.cpp).

The CPU counterpart of ``ops/hip.py``: every layer's CPU path runs these C++ kernels (blocked
AVX2 GEMM, per-sample im2col convolution, two-pass BatchNorm statistics, pooling with argmax
indices, fused losses, flat-buffer optimizers) on the native thread pool, in float32 or float64,
NCHW contiguous. ATen is only the test oracle (tests/test_cpu_backend.py).

Reference: src/ops/cpu/skernels.cpp / dkernels.cpp, src/math/cpu/sgemm.cpp / dgemm.cpp,
include/tensor/cpu/tensor_ops.hpp:283, src/nn/layers_impl/cpu/*_ops.cpp.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from ._ext import native

_DT = {torch.float32: 0, torch.float64: 1}
ACT_CODES = {"linear": 0, "relu": 1, "leaky_relu": 2, "elu": 3, "sigmoid": 4, "tanh": 5, "gelu": 6}
LOSS_CODES = {"crossentropy": 0, "softmax_crossentropy": 1, "logsoftmax_crossentropy": 1, "mse": 2, "mae": 3,
              "huber": 4, "soft_crossentropy": 5}


def C():
    return native().cpu


def dt(t: torch.Tensor) -> int:
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError(f"CPU backend computes in float32 / float64, got {t.dtype}") from None


def p(t: Optional[torch.Tensor]) -> int:
    return 0 if t is None else t.data_ptr()


def _c(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    if t is None:
        return None
    if t.is_cuda:
        raise TypeError("CPU backend got a GPU tensor")
    return t if t.is_contiguous() else t.contiguous()


def _same(ref: torch.Tensor, *ts):
    for t in ts:
        if t is not None and t.dtype != ref.dtype:
            raise TypeError(f"dtype mismatch: {t.dtype} vs {ref.dtype}")


def set_num_threads(n: int) -> None:
    C().set_num_threads(int(n))


def get_num_threads() -> int:
    return int(C().get_num_threads())


# ------------------------------------------------------------------ GEMM
def gemm(a: torch.Tensor, b: torch.Tensor, ta: bool = False, tb: bool = False, alpha: float = 1.0,
         beta: float = 0.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = alpha * op(a) @ op(b) + beta * out for 2-D row-major tensors."""
    a, b = _c(a), _c(b)
    _same(a, b)
    M, K = (a.shape[1], a.shape[0]) if ta else (a.shape[0], a.shape[1])
    K2, N = (b.shape[1], b.shape[0]) if tb else (b.shape[0], b.shape[1])
    if K != K2:
        raise ValueError(f"gemm: inner dims {K} vs {K2}")
    if out is None:
        out = torch.empty((M, N), dtype=a.dtype)
        beta = 0.0
    elif tuple(out.shape) != (M, N) or not out.is_contiguous():
        raise ValueError("gemm: out must be a contiguous [M, N] tensor")
    C().gemm(dt(a), ta, tb, M, N, K, float(alpha), a.data_ptr(), a.shape[1], b.data_ptr(), b.shape[1], float(beta),
             out.data_ptr(), N)
    return out


# ------------------------------------------------------------------ generic elementwise / reduce
def elementwise(mode: int, op: int, a, b=None, out=None, s0=0.0, s1=0.0):
    a = _c(a)
    b = _c(b)
    _same(a, b)
    if b is not None and b.numel() != a.numel():
        raise ValueError("size mismatch")
    if out is None:
        out = torch.empty_like(a)
    C().elementwise(dt(a), mode, op, a.data_ptr(), p(b), out.data_ptr(), a.numel(), float(s0), float(s1))
    return out


def ternary(op: int, a, b, c):
    a, b = _c(a), _c(b)
    _same(a, b, c)
    if not c.is_contiguous():
        raise ValueError("in-place target must be contiguous")
    C().elementwise(dt(a), 3, op, a.data_ptr(), b.data_ptr(), c.data_ptr(), a.numel(), 0.0, 0.0)
    return c


def axpy(alpha, x, y):
    x = _c(x)
    _same(x, y)
    C().elementwise(dt(x), 4, 0, x.data_ptr(), 0, y.data_ptr(), x.numel(), float(alpha), 0.0)
    return y


def reduce(op: int, a, b=None) -> torch.Tensor:
    a, b = _c(a), _c(b)
    v = C().reduce(dt(a), op, a.data_ptr(), p(b), a.numel())
    return torch.tensor([v], dtype=a.dtype)


def fill_random(a: torch.Tensor, lo: float, hi: float, seed: int, normal: bool) -> torch.Tensor:
    if not a.is_contiguous():
        raise ValueError("fill target must be contiguous")
    C().fill_random(dt(a), a.data_ptr(), a.numel(), int(seed) & ((1 << 64) - 1), float(lo), float(hi), int(normal))
    return a


def transpose_2d(a, rows, cols, batch=1):
    a = _c(a)
    out = torch.empty(batch * rows * cols, dtype=a.dtype)
    C().transpose2d(dt(a), a.data_ptr(), out.data_ptr(), batch, rows, cols)
    return out.view(batch, cols, rows) if batch > 1 else out.view(cols, rows)


def swap01(a: torch.Tensor) -> torch.Tensor:
    """[A][B][H][W] -> [B][A][H][W] (NCHW <-> CNHW)."""
    a = _c(a)
    A, B, H, W = a.shape
    out = torch.empty((B, A, H, W), dtype=a.dtype)
    C().swap01(dt(a), a.data_ptr(), out.data_ptr(), A, B, H * W)
    return out


def pad2d(x, ph, pw, value=0.0):
    x = _c(x)
    N, Cc, H, W = x.shape
    y = torch.empty((N, Cc, H + 2 * ph, W + 2 * pw), dtype=x.dtype)
    C().pad2d(dt(x), x.data_ptr(), y.data_ptr(), N * Cc, H, W, ph, pw, float(value))
    return y


def crop2d(x, top, left, oh, ow):
    x = _c(x)
    N, Cc, H, W = x.shape
    if top < 0 or left < 0 or top + oh > H or left + ow > W:
        raise ValueError("crop window outside the input")
    y = torch.empty((N, Cc, oh, ow), dtype=x.dtype)
    C().crop2d(dt(x), x.data_ptr(), y.data_ptr(), N * Cc, H, W, top, left, oh, ow)
    return y


def _odim(i, k, s, pd):
    return (i + 2 * pd - k) // s + 1


def im2col(x, kh, kw, sh, sw, ph, pw):
    """[C*KH*KW, N*OH*OW] column matrix (the reference layout)."""
    x = _c(x)
    N, Cc, H, W = x.shape
    OH, OW = _odim(H, kh, sh, ph), _odim(W, kw, sw, pw)
    col = torch.empty((Cc * kh * kw, N * OH * OW), dtype=x.dtype)
    C().im2col(dt(x), x.data_ptr(), col.data_ptr(), N, Cc, H, W, kh, kw, sh, sw, ph, pw)
    return col


def col2im(col, shape, kh, kw, sh, sw, ph, pw):
    col = _c(col)
    N, Cc, H, W = shape
    x = torch.empty((N, Cc, H, W), dtype=col.dtype)
    C().col2im(dt(col), col.data_ptr(), x.data_ptr(), N, Cc, H, W, kh, kw, sh, sw, ph, pw)
    return x


# ------------------------------------------------------------------ layers
def conv2d_fwd(x, w, bias, stride, pad):
    x, w, bias = _c(x), _c(w), _c(bias)
    _same(x, w, bias)
    N, Ci, H, W = x.shape
    Co, Ci2, KH, KW = w.shape
    if Ci != Ci2:
        raise ValueError(f"conv2d: {Ci} input channels, weights expect {Ci2}")
    OH, OW = _odim(H, KH, stride[0], pad[0]), _odim(W, KW, stride[1], pad[1])
    y = torch.empty((N, Co, OH, OW), dtype=x.dtype)
    C().conv2d_fwd(dt(x), x.data_ptr(), w.data_ptr(), p(bias), y.data_ptr(), N, Ci, H, W, Co, KH, KW, stride[0],
                   stride[1], pad[0], pad[1])
    return y


def _bwd_dx(x, grad_w, grad_b, need_dx):
    """a conv backward's dx buffer (None without need_dx), after the accumulators' contiguity check"""
    for g in (grad_w, grad_b):
        if g is not None and not g.is_contiguous():
            raise ValueError("gradient accumulators must be contiguous")
    return torch.empty_like(x) if need_dx else None


def conv2d_bwd(x, w, dy, stride, pad, grad_w, grad_b=None, need_dx=True):
    """grad_w (+)= dW, grad_b (+)= sum(dy); returns dx (or None). grad_w/grad_b must be contiguous."""
    x, w, dy = _c(x), _c(w), _c(dy)
    _same(x, w, dy, grad_w, grad_b)
    N, Ci, H, W = x.shape
    Co, _, KH, KW = w.shape
    dx = _bwd_dx(x, grad_w, grad_b, need_dx)
    C().conv2d_bwd(dt(x), x.data_ptr(), w.data_ptr(), dy.data_ptr(), p(dx), grad_w.data_ptr(), p(grad_b), N, Ci, H, W,
                   Co, KH, KW, stride[0], stride[1], pad[0], pad[1])
    return dx


def depthwise_conv2d_fwd(x, w, bias, stride, pad):
    """Depthwise conv (groups = C, multiplier 1): w (C,1,KH,KW), bias [C] or None."""
    x, w, bias = _c(x), _c(w), _c(bias)
    _same(x, w, bias)
    N, Cc, H, W = x.shape
    C2, one, KH, KW = w.shape
    if C2 != Cc or one != 1:
        raise ValueError(f"depthwise_conv2d: {Cc} input channels, weights {tuple(w.shape)} (expected ({Cc}, 1, KH, KW))")
    OH, OW = _odim(H, KH, stride[0], pad[0]), _odim(W, KW, stride[1], pad[1])
    if OH < 1 or OW < 1:
        raise ValueError(f"depthwise_conv2d: kernel {KH}x{KW} does not fit the padded {H}x{W} input")
    y = torch.empty((N, Cc, OH, OW), dtype=x.dtype)
    C().depthwise_conv2d_fwd(dt(x), x.data_ptr(), w.data_ptr(), p(bias), y.data_ptr(), N, Cc, H, W, KH, KW, stride[0],
                             stride[1], pad[0], pad[1])
    return y


def depthwise_conv2d_bwd(x, w, dy, stride, pad, grad_w, grad_b=None, need_dx=True):
    """grad_w += dW, grad_b += sum(dy); returns dx (or None). grad_w/grad_b must be contiguous."""
    x, w, dy = _c(x), _c(w), _c(dy)
    _same(x, w, dy, grad_w, grad_b)
    N, Cc, H, W = x.shape
    _, _, KH, KW = w.shape
    OH, OW = _odim(H, KH, stride[0], pad[0]), _odim(W, KW, stride[1], pad[1])
    if tuple(w.shape[:2]) != (Cc, 1) or tuple(dy.shape) != (N, Cc, OH, OW):
        raise ValueError(f"depthwise_conv2d_bwd: x {tuple(x.shape)}, w {tuple(w.shape)}, dy {tuple(dy.shape)}")
    dx = _bwd_dx(x, grad_w, grad_b, need_dx)
    C().depthwise_conv2d_bwd(dt(x), x.data_ptr(), w.data_ptr(), dy.data_ptr(), p(dx), grad_w.data_ptr(), p(grad_b), N,
                             Cc, H, W, KH, KW, stride[0], stride[1], pad[0], pad[1])
    return dx


def _grouped_geom(what, x, w, groups, stride, pad):
    N, Cc, H, W = x.shape
    Co, Cig, KH, KW = w.shape
    if groups < 1 or Cc % groups or Co % groups or Cig != Cc // groups:
        raise ValueError(f"{what}: {Cc} input channels, weights {tuple(w.shape)}, groups {groups} (expected "
                         f"({Co}, {Cc}/groups, KH, KW) with groups dividing both channel counts)")
    OH, OW = _odim(H, KH, stride[0], pad[0]), _odim(W, KW, stride[1], pad[1])
    if OH < 1 or OW < 1:
        raise ValueError(f"{what}: kernel {KH}x{KW} does not fit the padded {H}x{W} input")
    return N, Cc, H, W, Co, KH, KW, OH, OW


def grouped_conv2d_fwd(x, w, bias, stride, pad, groups):
    """Grouped conv (F.conv2d(groups=G)): w (Co,C/G,KH,KW), bias [Co] or None."""
    x, w, bias = _c(x), _c(w), _c(bias)
    _same(x, w, bias)
    N, Cc, H, W, Co, KH, KW, OH, OW = _grouped_geom("grouped_conv2d", x, w, groups, stride, pad)
    y = torch.empty((N, Co, OH, OW), dtype=x.dtype)
    C().grouped_conv2d_fwd(dt(x), x.data_ptr(), w.data_ptr(), p(bias), y.data_ptr(), N, Cc, H, W, Co, groups, KH, KW,
                           stride[0], stride[1], pad[0], pad[1])
    return y


def grouped_conv2d_bwd(x, w, dy, stride, pad, groups, grad_w, grad_b=None, need_dx=True):
    """grad_w += dW, grad_b += sum(dy); returns dx (or None). grad_w/grad_b must be contiguous."""
    x, w, dy = _c(x), _c(w), _c(dy)
    _same(x, w, dy, grad_w, grad_b)
    N, Cc, H, W, Co, KH, KW, OH, OW = _grouped_geom("grouped_conv2d_bwd", x, w, groups, stride, pad)
    if tuple(dy.shape) != (N, Co, OH, OW):
        raise ValueError(f"grouped_conv2d_bwd: x {tuple(x.shape)}, w {tuple(w.shape)}, dy {tuple(dy.shape)}")
    dx = _bwd_dx(x, grad_w, grad_b, need_dx)
    C().grouped_conv2d_bwd(dt(x), x.data_ptr(), w.data_ptr(), dy.data_ptr(), p(dx), grad_w.data_ptr(), p(grad_b), N,
                           Cc, H, W, Co, groups, KH, KW, stride[0], stride[1], pad[0], pad[1])
    return dx


def dense_fwd(x2d, w2d, bias):
    x2d, w2d, bias = _c(x2d), _c(w2d), _c(bias)
    _same(x2d, w2d, bias)
    N, In = x2d.shape
    Out = w2d.shape[0]
    y = torch.empty((N, Out), dtype=x2d.dtype)
    C().dense_fwd(dt(x2d), x2d.data_ptr(), w2d.data_ptr(), p(bias), y.data_ptr(), N, In, Out)
    return y


def dense_bwd(x2d, w2d, dy2d, grad_w, grad_b=None, need_dx=True):
    x2d, w2d, dy2d = _c(x2d), _c(w2d), _c(dy2d)
    _same(x2d, w2d, dy2d, grad_w, grad_b)
    N, In = x2d.shape
    Out = w2d.shape[0]
    dx = torch.empty_like(x2d) if need_dx else None
    C().dense_bwd(dt(x2d), x2d.data_ptr(), w2d.data_ptr(), dy2d.data_ptr(), p(dx), grad_w.data_ptr(), p(grad_b), N,
                  In, Out)
    return dx


def batchnorm_fwd(x, gamma, beta, eps, training, running_mean, running_var, momentum, relu=False, residual=None):
    """Returns (y, mean, istd). Training: batch statistics (two-pass), running stats updated with
    the unbiased variance; eval: running statistics."""
    x, residual = _c(x), _c(residual)
    _same(x, gamma, beta, residual, running_mean, running_var)
    N, Cc, H, W = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(Cc, dtype=x.dtype)
    istd = torch.empty(Cc, dtype=x.dtype)
    C().batchnorm_fwd(dt(x), x.data_ptr(), y.data_ptr(), N, Cc, H * W, p(gamma), p(beta), float(eps), int(training),
                      p(running_mean), p(running_var), float(momentum), mean.data_ptr(), istd.data_ptr(), int(relu),
                      p(residual))
    return y, mean, istd


def batchnorm_bwd(x, dy, yout, mean, istd, gamma, dgamma, dbeta, training=True, want_masked=False, need_dx=True):
    """Returns (dx, masked_dy). ``yout`` given: dy is masked by (yout > 0) (fused ReLU)."""
    x, dy, yout = _c(x), _c(dy), _c(yout)
    _same(x, dy, yout, mean, istd, gamma, dgamma, dbeta)
    N, Cc, H, W = x.shape
    dx = torch.empty_like(x) if need_dx else None
    masked = torch.empty_like(dy) if want_masked else None
    C().batchnorm_bwd(dt(x), x.data_ptr(), dy.data_ptr(), p(yout), mean.data_ptr(), istd.data_ptr(), p(gamma), p(dx),
                      p(dgamma), p(dbeta), p(masked), N, Cc, H * W, int(training))
    return dx, masked


def groupnorm_fwd(x, G, gamma, beta, eps):
    x = _c(x)
    _same(x, gamma, beta)
    N, Cc, H, W = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(N * G, dtype=x.dtype)
    istd = torch.empty(N * G, dtype=x.dtype)
    C().groupnorm_fwd(dt(x), x.data_ptr(), y.data_ptr(), N, Cc, H * W, G, p(gamma), p(beta), float(eps),
                      mean.data_ptr(), istd.data_ptr())
    return y, mean, istd


def groupnorm_bwd(x, dy, G, gamma, mean, istd, dgamma, dbeta):
    x, dy = _c(x), _c(dy)
    _same(x, dy, gamma, mean, istd, dgamma, dbeta)
    N, Cc, H, W = x.shape
    dx = torch.empty_like(x)
    C().groupnorm_bwd(dt(x), x.data_ptr(), dy.data_ptr(), mean.data_ptr(), istd.data_ptr(), p(gamma), dx.data_ptr(),
                      p(dgamma), p(dbeta), N, Cc, H * W, G)
    return dx


def _nchw_rows(x):
    """(N, C, HW) of a [N, C, ...] tensor (a 2-D [N, F] input: HW = 1)."""
    if x.dim() < 2:
        raise ValueError(f"expected a [N, C, ...] tensor, got {tuple(x.shape)}")
    N, Cc = x.shape[0], x.shape[1]
    return N, Cc, x.numel() // max(N * Cc, 1)


def layernorm_fwd(x, gamma, beta, eps):
    """Channel LayerNorm: every (n, position) of x [N, C, ...] over its C channels. Returns
    (y, mean, rstd), the statistics as [N * HW]."""
    x = _c(x)
    _same(x, gamma, beta)
    N, Cc, HW = _nchw_rows(x)
    y = torch.empty_like(x)
    mean = torch.empty(N * HW, dtype=x.dtype)
    rstd = torch.empty(N * HW, dtype=x.dtype)
    C().layernorm_fwd(dt(x), x.data_ptr(), y.data_ptr(), N, Cc, HW, p(gamma), p(beta), float(eps), mean.data_ptr(),
                      rstd.data_ptr())
    return y, mean, rstd


def layernorm_bwd(x, dy, gamma, mean, rstd, dgamma, dbeta):
    """dgamma += sum dy xhat, dbeta += sum dy; returns dx."""
    x, dy = _c(x), _c(dy)
    _same(x, dy, gamma, mean, rstd, dgamma, dbeta)
    N, Cc, HW = _nchw_rows(x)
    dx = torch.empty_like(x)
    C().layernorm_bwd(dt(x), x.data_ptr(), dy.data_ptr(), mean.data_ptr(), rstd.data_ptr(), p(gamma), dx.data_ptr(),
                      p(dgamma), p(dbeta), N, Cc, HW)
    return dx


def layer_scale_fwd(x, gamma, residual=None):
    """y = gamma[c] * x (+ residual)."""
    x, residual = _c(x), _c(residual)
    _same(x, gamma, residual)
    N, Cc, HW = _nchw_rows(x)
    if gamma.numel() != Cc or (residual is not None and residual.shape != x.shape):
        raise ValueError(f"layer_scale: x {tuple(x.shape)}, gamma {gamma.numel()} values")
    y = torch.empty_like(x)
    C().layer_scale_fwd(dt(x), x.data_ptr(), gamma.data_ptr(), p(residual), y.data_ptr(), N, Cc, HW)
    return y


def layer_scale_bwd(x, dy, gamma, dgamma, need_dx=True):
    """dgamma += sum dy x; returns dx = gamma[c] * dy (or None)."""
    x, dy = _c(x), _c(dy)
    _same(x, dy, gamma, dgamma)
    N, Cc, HW = _nchw_rows(x)
    dx = torch.empty_like(x) if need_dx else None
    C().layer_scale_bwd(dt(x), x.data_ptr(), dy.data_ptr(), gamma.data_ptr(), p(dx), p(dgamma), N, Cc, HW)
    return dx


def maxpool_fwd(x, k, s, pd) -> Tuple[torch.Tensor, torch.Tensor]:
    x = _c(x)
    N, Cc, H, W = x.shape
    OH, OW = _odim(H, k[0], s[0], pd[0]), _odim(W, k[1], s[1], pd[1])
    y = torch.empty((N, Cc, OH, OW), dtype=x.dtype)
    idx = torch.empty((N, Cc, OH, OW), dtype=torch.int32)
    C().maxpool_fwd(dt(x), x.data_ptr(), y.data_ptr(), idx.data_ptr(), N * Cc, H, W, k[0], k[1], s[0], s[1], pd[0],
                    pd[1])
    return y, idx


def maxpool_bwd(dy, idx, in_shape):
    dy, idx = _c(dy), _c(idx)
    N, Cc, H, W = in_shape
    dx = torch.empty((N, Cc, H, W), dtype=dy.dtype)
    C().maxpool_bwd(dt(dy), dy.data_ptr(), idx.data_ptr(), dx.data_ptr(), N * Cc, H, W, dy.shape[2], dy.shape[3])
    return dx


def avgpool_fwd(x, k, s, pd):
    x = _c(x)
    N, Cc, H, W = x.shape
    OH, OW = _odim(H, k[0], s[0], pd[0]), _odim(W, k[1], s[1], pd[1])
    y = torch.empty((N, Cc, OH, OW), dtype=x.dtype)
    C().avgpool_fwd(dt(x), x.data_ptr(), y.data_ptr(), N * Cc, H, W, k[0], k[1], s[0], s[1], pd[0], pd[1])
    return y


def avgpool_bwd(dy, in_shape, k, s, pd):
    dy = _c(dy)
    N, Cc, H, W = in_shape
    dx = torch.empty((N, Cc, H, W), dtype=dy.dtype)
    C().avgpool_bwd(dt(dy), dy.data_ptr(), dx.data_ptr(), N * Cc, H, W, k[0], k[1], s[0], s[1], pd[0], pd[1])
    return dx


def act_fwd(x, kind, alpha=0.0):
    x = _c(x)
    y = torch.empty_like(x)
    C().act_fwd(dt(x), ACT_CODES[kind], x.data_ptr(), y.data_ptr(), x.numel(), float(alpha))
    return y


def act_bwd(x, dy, kind, alpha=0.0):
    x, dy = _c(x), _c(dy)
    _same(x, dy)
    dx = torch.empty_like(x)
    C().act_bwd(dt(x), ACT_CODES[kind], x.data_ptr(), dy.data_ptr(), dx.data_ptr(), x.numel(), float(alpha))
    return dx


def _nchw(x):
    N, Cc = x.shape[0], x.shape[1]
    return N, Cc, x.numel() // max(N * Cc, 1)


def softmax_channels(x):
    x = _c(x)
    y = torch.empty_like(x)
    C().softmax_channels(dt(x), x.data_ptr(), y.data_ptr(), *_nchw(x))
    return y


def softmax_channels_bwd(y, dy):
    y, dy = _c(y), _c(dy)
    dx = torch.empty_like(y)
    C().softmax_channels_bwd(dt(y), y.data_ptr(), dy.data_ptr(), dx.data_ptr(), *_nchw(y))
    return dx


def loss_fused(pred2d, target2d=None, labels=None, kind="softmax_crossentropy", param=0.0, want_grad=True):
    """(loss[1], grad | None, correct[1] int32) — the CPU twin of ``hip.loss_fused``."""
    pred2d = _c(pred2d)
    N, Cn = pred2d.shape
    tgt = _c(target2d.to(pred2d.dtype)) if target2d is not None else None
    lab = _c(labels.to(torch.int64)) if labels is not None else None
    grad = torch.empty_like(pred2d) if want_grad else None
    l, cor = C().loss_fused(dt(pred2d), LOSS_CODES[kind], pred2d.data_ptr(), p(tgt), p(lab), p(grad), N, Cn,
                            float(param))
    return (torch.tensor([l], dtype=pred2d.dtype), grad, torch.tensor([cor], dtype=torch.int32))


def sgd_step(p_, g, vel, lr, momentum):
    C().sgd_step(dt(p_), p_.data_ptr(), g.data_ptr(), p(vel), p_.numel(), float(lr), float(momentum))


def adam_step(p_, g, m, v, lr, b1, b2, eps, bc1, bc2, wd, decoupled):
    C().adam_step(dt(p_), p_.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p_.numel(), float(lr), float(b1),
                  float(b2), float(eps), float(bc1), float(bc2), float(wd), int(decoupled))


def adam_step_nodecay(p_, g, m, v, lr, b1, b2, eps, bc1, bc2, wd, decoupled, nodecay):
    """:func:`adam_step` with ``wd = 0`` for every 64-element block of the flat buffer whose byte in
    ``nodecay`` (uint8, ``ceil(n / 64)`` entries) is set."""
    if nodecay.dtype != torch.uint8 or not nodecay.is_contiguous() or nodecay.numel() * 64 < p_.numel():
        raise ValueError("adam_step_nodecay: the block table is uint8 with one entry per 64 elements")
    C().adam_step_nodecay(dt(p_), p_.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p_.numel(), float(lr),
                          float(b1), float(b2), float(eps), float(bc1), float(bc2), float(wd), int(decoupled),
                          nodecay.data_ptr())


def grad_sumsq(g) -> float:
    """Sum of ``g**2`` over a flat float32 / float64 buffer, in a fixed order (double partials)."""
    g = _c(g)
    return float(C().grad_sumsq(dt(g), g.data_ptr(), g.numel()))


def _nodecay_ptr(who, nodecay, n):
    if nodecay is None:
        return 0
    if nodecay.dtype != torch.uint8 or not nodecay.is_contiguous() or nodecay.numel() * 64 < n:
        raise ValueError(f"{who}: the block table is uint8 with one entry per 64 elements")
    return nodecay.data_ptr()


def adam_step_tail(p_, g, m, v, lr, b1, b2, eps, bc1, bc2, wd, decoupled, nodecay=None, coef=None, ema=None,
                   ema_decay=0.0):
    """:func:`adam_step` with three optional inputs: ``nodecay`` (the block table of
    :func:`adam_step_nodecay`), ``coef`` (the clip coefficient: the step takes ``g * coef``, ``g`` is
    left as it is) and ``ema`` (``ema = d ema + (1 - d) p_new``)."""
    _same(p_, g, m, v, ema)
    C().adam_step_tail(dt(p_), p_.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p_.numel(), float(lr),
                       float(b1), float(b2), float(eps), float(bc1), float(bc2), float(wd), int(decoupled),
                       _nodecay_ptr("adam_step_tail", nodecay, p_.numel()), coef is not None,
                       float(coef if coef is not None else 1.0), p(ema), float(ema_decay))


def sgd_step_tail(p_, g, vel, lr, momentum, coef=None, ema=None, ema_decay=0.0):
    """:func:`sgd_step` with the clip coefficient and the EMA buffer, both optional."""
    _same(p_, g, vel, ema)
    C().sgd_step_tail(dt(p_), p_.data_ptr(), g.data_ptr(), p(vel), p_.numel(), float(lr), float(momentum),
                      coef is not None, float(coef if coef is not None else 1.0), p(ema), float(ema_decay))


def _layerwise_args(who, n, tables, trust):
    if tables.cover > n:
        raise ValueError(f"{who}: the chunk table reaches element {tables.cover}, the buffers hold {n} "
                         f"(chunks are whole 64-element blocks inside the buffers)")
    if trust.dtype != torch.float64 or not trust.is_contiguous() or trust.numel() < 3 * tables.nsegs:
        raise ValueError(f"{who}: trust is a float64 tensor of at least {3 * tables.nsegs} elements")
    return (tables.chunks.data_ptr(), tables.nchunks, tables.segs.data_ptr(), tables.nsegs, trust.data_ptr())


def lamb_step(p_, g, m, v, lr, b1, b2, eps, bc1, bc2, wd, tables, trust, coef=None, ema=None, ema_decay=0.0):
    """One LAMB step over a flat float32 / float64 buffer, driven by the GPU's segment / chunk tables
    (``SegmentTables``). ``trust`` (float64, ``[3 * nsegs]``) receives the trust ratios, then the pairs
    ``{sum p^2, sum r^2}``. ``coef`` / ``ema`` as in :func:`adam_step_tail`."""
    _same(p_, g, m, v, ema)
    C().lamb_step(dt(p_), p_.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p_.numel(), float(lr), float(b1),
                  float(b2), float(eps), float(bc1), float(bc2), float(wd), coef is not None,
                  float(coef if coef is not None else 1.0), p(ema), float(ema_decay),
                  *_layerwise_args("lamb_step", p_.numel(), tables, trust))


def lars_step(p_, g, vel, lr, momentum, wd, trust_coefficient, eps, tables, trust, coef=None, ema=None,
              ema_decay=0.0):
    """One LARS step over a flat buffer (``vel`` None: no momentum); see :func:`lamb_step`."""
    _same(p_, g, vel, ema)
    C().lars_step(dt(p_), p_.data_ptr(), g.data_ptr(), p(vel), p_.numel(), float(lr), float(momentum), float(wd),
                  float(trust_coefficient), float(eps), coef is not None, float(coef if coef is not None else 1.0),
                  p(ema), float(ema_decay), *_layerwise_args("lars_step", p_.numel(), tables, trust))


def ema_swap(a, b):
    """Exchange two flat buffers of one dtype and size in place; twice restores every bit."""
    _same(a, b)
    if a.numel() != b.numel() or not a.is_contiguous() or not b.is_contiguous() or a.data_ptr() == b.data_ptr():
        raise ValueError("ema_swap: two distinct contiguous buffers of one size")
    C().ema_swap(dt(a), a.data_ptr(), b.data_ptr(), a.numel())


def mix_plan(seed: int, step: int, H: int, W: int, mixup_alpha: float, cutmix_alpha: float, prob: float = 1.0,
             switch_prob: float = 0.5):
    """The Mixup / CutMix draw of training batch ``step`` (from 1): ``(mode, lam, yl, yh, xl, xh)``,
    mode 0 none / 1 Mixup / 2 CutMix. A pure function of its arguments (csrc/native mix_plan), the
    one both front ends call."""
    return tuple(C().mix_plan(int(seed) & ((1 << 64) - 1), int(step) & ((1 << 64) - 1), int(H), int(W),
                              float(mixup_alpha), float(cutmix_alpha), float(prob), float(switch_prob)))


def mix_batch(x, labels, target, mode, lam, box, num_classes):
    """Mixup (mode 1) / CutMix (mode 2, ``box = (yl, yh, xl, xh)``) of ``x`` [B, C, H, W] with its
    reversed batch, in place, and the dense float32 ``target`` [B, K] written whole. The rounding is
    the GPU kernel's: the two backends agree bit for bit."""
    if x.dim() != 4 or not x.is_contiguous() or x.is_cuda:
        raise ValueError("mix_batch: x is a contiguous CPU [B, C, H, W] tensor")
    B, Cn, H, W = x.shape
    K = int(num_classes)
    C().mix_check(B, Cn, H, W, K, int(mode), float(lam), *map(int, box))
    if labels.dtype != torch.int64 or labels.shape != (B,) or not labels.is_contiguous():
        raise ValueError("mix_batch: labels are int64 [B]")
    if target.dtype != torch.float32 or target.shape != (B, K) or not target.is_contiguous():
        raise ValueError("mix_batch: target is a contiguous float32 [B, num_classes] tensor")
    C().mix_batch(dt(x), x.data_ptr(), labels.data_ptr(), target.data_ptr(), B, Cn, H, W, int(mode), float(lam),
                  *map(int, box), K)
    return x, target


def drop_path_mask(seed: int, draw: int, n: int, p_drop: float) -> torch.Tensor:
    """The stochastic-depth mask of (seed, draw): ``n`` float32 values, 0 or 1 / (1 - p). The same
    function as the GPU kernel's (csrc/kernels/droppath.hip), bit for bit."""
    return torch.tensor(C().drop_path_mask(int(seed) & ((1 << 64) - 1), int(draw) & ((1 << 64) - 1), int(n),
                                           float(p_drop)), dtype=torch.float32)


def drop_path_scale(x, mask):
    """y[n] = mask[n] * x[n] (mask float32 [N]); a dropped sample is not read."""
    x = _c(x)
    if mask.dtype != torch.float32 or mask.numel() != x.shape[0] or not mask.is_contiguous():
        raise ValueError(f"drop_path_scale: x {tuple(x.shape)}, mask {tuple(mask.shape)} {mask.dtype}")
    y = torch.empty_like(x)
    C().drop_path_scale(dt(x), x.data_ptr(), mask.data_ptr(), y.data_ptr(), x.shape[0], x.numel() // max(x.shape[0], 1))
    return y
