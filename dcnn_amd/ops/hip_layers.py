"""Dense layers, pooling, activations, loss, optimizer steps and layout helpers on the HIP kernels."""
from __future__ import annotations

import torch

from ..runtime import arena as _arena
from . import fusion
from ._ext import dt_code, kernels, ptr, stream_ptr
from .hip_base import (BF16, CL, F32, PLAIN, _check_act, _empty, _empty_like, _g2_ok, _nbytes,
                       _rec, _reduce_wb, _ticket, conv_out_hw, pool_out_hw)
from .hip_norm import _ln_like, ln_rows


def dense_fwd(x2d, w2d, bias):
    """y[N,Out] = x[N,In] . w[Out,In]^T + b   (bf16 in/out, fp32 accumulate)."""
    N, In = x2d.shape
    Out = w2d.shape[0]
    if x2d.dtype == F32:
        y = _empty((N, Out), F32, x2d.device)
        kernels().gemm_g2_plain(1, x2d.data_ptr(), w2d.data_ptr(), y.data_ptr(), _nbytes(x2d), _nbytes(w2d), N, Out, In,
                                ptr(bias), 0, 0, 0, 0, 0, stream_ptr())
        return y
    y = _empty((N, Out), BF16, x2d.device)
    if _g2_ok(In, Out):
        kernels().gemm_g2_plain(0, x2d.data_ptr(), w2d.data_ptr(), y.data_ptr(), _nbytes(x2d), _nbytes(w2d), N, Out, In,
                                ptr(bias), 0, 0, 0, 0, 0, stream_ptr())
        return y
    kernels().gemm_nt(x2d.data_ptr(), w2d.data_ptr(), y.data_ptr(), N, Out, In, In, In, Out, PLAIN,
                      0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 0, 0, ptr(bias), 0, 0, 0, 0, stream_ptr())
    return y


def dense_dgrad(dy2d, wt2d):
    """dx[N,In] = dy[N,Out] . w[Out,In]   with wt2d = w^T stored [In][Out]."""
    N, Out = dy2d.shape
    In = wt2d.shape[0]
    if dy2d.dtype == F32:
        dx = _empty((N, In), F32, dy2d.device)
        kernels().gemm_g2_plain(1, dy2d.data_ptr(), wt2d.data_ptr(), dx.data_ptr(), _nbytes(dy2d), _nbytes(wt2d), N, In,
                                Out, 0, 0, 0, 0, 0, 0, stream_ptr())
        return dx
    dx = _empty((N, In), BF16, dy2d.device)
    if _g2_ok(Out, In):
        kernels().gemm_g2_plain(0, dy2d.data_ptr(), wt2d.data_ptr(), dx.data_ptr(), _nbytes(dy2d), _nbytes(wt2d), N, In,
                                Out, 0, 0, 0, 0, 0, 0, stream_ptr())
        return dx
    kernels().gemm_nt(dy2d.data_ptr(), wt2d.data_ptr(), dx.data_ptr(), N, In, Out, Out, Out, In, PLAIN,
                      0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, stream_ptr())
    return dx


def dense_wgrad(dy2d, x2d, grad_w, grad_b=None):
    K = kernels()
    N, Out = dy2d.shape
    In = x2d.shape[1]
    st = stream_ptr()
    if dy2d.dtype == F32:
        splits = K.gemm_t2f_splits(Out, In, N)
        slab = _empty((splits, Out, In), F32, x2d.device)
        bslab = _empty((splits, Out), F32, x2d.device) if grad_b is not None else None
        K.gemm_t2_plain(1, dy2d.data_ptr(), x2d.data_ptr(), slab.data_ptr(), ptr(bslab), 0, 0, Out, In, N, splits, st)
    elif _g2_ok(In, Out):
        splits = K.gemm_t2_splits(Out, In, N)
        slab = _empty((splits, Out, In), F32, x2d.device)
        bslab = _empty((splits, Out), F32, x2d.device) if grad_b is not None else None
        K.gemm_t2_plain(0, dy2d.data_ptr(), x2d.data_ptr(), slab.data_ptr(), ptr(bslab), _nbytes(dy2d), _nbytes(x2d),
                        Out, In, N, splits, st)
    else:
        splits = K.gemm_tn_splits(Out, In, N)
        slab = _empty((splits, Out, In), F32, x2d.device)
        bslab = _empty((splits, Out), F32, x2d.device) if grad_b is not None else None
        K.gemm_tn(dy2d.data_ptr(), x2d.data_ptr(), slab.data_ptr(), ptr(bslab), Out, In, N, PLAIN,
                  0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 0, 0, In, splits, st)
    _reduce_wb(K, slab, grad_w, Out * In, bslab, grad_b, Out, splits, st)


# ------------------------------------------------------------------------------ pooling
def maxpool_fwd(x, ph, pw, sh, sw, pdh, pdw):
    _check_act(x, "maxpool")
    N, C, H, W = x.shape
    OH, OW = pool_out_hw(H, W, ph, pw, sh, sw, pdh, pdw)
    y = _empty((N, C, OH, OW), x.dtype, x.device, True)
    idx = _empty((N, OH, OW, C), torch.uint8, x.device)
    assert ph * pw <= 256
    kernels().maxpool_fwd(dt_code(x.dtype), x.data_ptr(), y.data_ptr(), idx.data_ptr(), N, H, W, C, OH, OW, ph, pw,
                          sh, sw, pdh, pdw, stream_ptr())
    return y, idx


def maxpool_bwd(dy, idx, x_shape, ph, pw, sh, sw, pdh, pdw, *, ypool=None, bnb=None):
    """Gather-form max-pool backward. With ``bnb`` (the BatchNorm+ReLU that produced the pool's
    input, see :class:`BnbRequest`) and the pool output ``ypool``, the ReLU mask (pooled value > 0)
    and that BatchNorm's backward statistics are fused in (``dx._bnb`` attached)."""
    N, C, H, W = x_shape
    OH, OW = dy.shape[2], dy.shape[3]
    K = kernels()
    dx = _empty((N, C, H, W), dy.dtype, dy.device, True)
    g = (N, H, W, C, OH, OW, ph, pw, sh, sw, pdh, pdw)
    # the kernel masks with (pooled value > 0): only valid when a ReLU sits between BN and pool
    if (bnb is not None and fusion.BNB and (bnb.y is not None or bnb.pooled) and ypool is not None and dy.dtype == BF16 and bnb.x.dtype == BF16
            and tuple(bnb.x.shape) == (N, C, H, W) and bnb.x.is_contiguous(memory_format=CL)
            and K.maxpool_bwd_bnb_supported(*g)):
        rows = K.maxpool_bwd_bnb_rows(*g)
        slab = _empty((rows, 2, C), F32, dy.device)
        sums = _empty((2 * C,), F32, dy.device)  # zeroed in-kernel
        K.maxpool_bwd_bnb(dy.data_ptr(), idx.data_ptr(), ypool.data_ptr(), bnb.x.data_ptr(), bnb.mean.data_ptr(),
                          bnb.istd.data_ptr(), dx.data_ptr(), *g, slab.data_ptr(), sums.data_ptr(), stream_ptr())
        dx._bnb = (bnb.bn, slab, rows, sums)
        return dx
    K.maxpool_bwd(dt_code(dy.dtype), dy.data_ptr(), idx.data_ptr(), dx.data_ptr(), *g, stream_ptr())
    return dx


def avgpool_fwd(x, ph, pw, sh, sw, pdh, pdw):
    _check_act(x, "avgpool")
    N, C, H, W = x.shape
    OH, OW = pool_out_hw(H, W, ph, pw, sh, sw, pdh, pdw)
    y = _empty((N, C, OH, OW), x.dtype, x.device, True)
    kernels().avgpool_fwd(dt_code(x.dtype), x.data_ptr(), y.data_ptr(), N, H, W, C, OH, OW, ph, pw, sh, sw, pdh, pdw,
                          stream_ptr())
    return y


def avgpool_bwd(dy, x_shape, ph, pw, sh, sw, pdh, pdw):
    N, C, H, W = x_shape
    OH, OW = dy.shape[2], dy.shape[3]
    dy = dy.contiguous(memory_format=CL)
    dx = _empty((N, C, H, W), dy.dtype, dy.device, True)
    kernels().avgpool_bwd(dt_code(dy.dtype), dy.data_ptr(), dx.data_ptr(), N, H, W, C, OH, OW, ph, pw, sh, sw, pdh,
                          pdw, stream_ptr())
    return dx


# ------------------------------------------------------------------------------ activations
ACT_CODES = {"relu": 0, "leaky_relu": 1, "elu": 2, "sigmoid": 3, "tanh": 4, "linear": 5, "gelu": 6}


def act_fwd(x, kind, alpha=0.01):
    y = _empty_like(x)
    kernels().act_fwd(dt_code(x.dtype), x.data_ptr(), y.data_ptr(), x.numel(), ACT_CODES[kind], float(alpha),
                      stream_ptr())
    return y


def act_bwd(x, dy, kind, alpha=0.01):
    dy = dy.contiguous(memory_format=CL) if x.dim() == 4 and x.is_contiguous(memory_format=CL) else dy.contiguous()
    dx = _empty_like(x)
    kernels().act_bwd(dt_code(x.dtype), x.data_ptr(), dy.data_ptr(), dx.data_ptr(), x.numel(), ACT_CODES[kind],
                      float(alpha), stream_ptr())
    return dx


def lscale_fwd(x, gamma, residual=None):
    """LayerScale (lnorm.hip): y = gamma[c] * x (+ residual, a same-shape activation, added in
    the same store); gamma fp32 [C]. x: 4-D channels_last or contiguous 2-D [R, C]."""
    R, C = ln_rows(x, "lscale_fwd")
    assert gamma.dtype == F32 and gamma.numel() == C and gamma.is_contiguous(), "lscale_fwd: gamma fp32 [C]"
    if residual is not None:
        _ln_like(residual, x, "lscale_fwd.residual")
    _rec("lscale_fwd", x=tuple(x.shape), residual=residual is not None)
    y = _empty_like(x)
    kernels().lscale_fwd(dt_code(x.dtype), x.data_ptr(), gamma.data_ptr(), ptr(residual), y.data_ptr(), R, C,
                         stream_ptr())
    return y


def lscale_bwd(dy, x, gamma, dgamma):
    """dx = gamma[c] * dy; dgamma += sum dy * x (fp32 [C]), summed in a fixed order through a
    per-workgroup slab (bit-reproducible)."""
    R, C = ln_rows(x, "lscale_bwd")
    _ln_like(dy, x, "lscale_bwd.dy")
    for t in (gamma, dgamma):
        assert t.dtype == F32 and t.numel() == C and t.is_contiguous(), "lscale_bwd: gamma / dgamma fp32 [C]"
    _rec("lscale_bwd", x=tuple(x.shape))
    K = kernels()
    dx = _empty_like(x)
    ws = _empty((K.ln_partial_rows(R, C), C), F32, x.device)
    K.lscale_bwd(dt_code(x.dtype), dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), dx.data_ptr(), dgamma.data_ptr(), R, C,
                 ws.data_ptr(), stream_ptr())
    return dx


def softmax_channels(x):
    """softmax over dim 1 of an NCHW-logical / NHWC-physical tensor (channel innermost)."""
    N, C = x.shape[0], x.shape[1]
    rows = x.numel() // C
    y = _empty_like(x)
    kernels().softmax_rows(dt_code(x.dtype), x.data_ptr(), y.data_ptr(), rows, C, stream_ptr())
    return y


def softmax_channels_bwd(y, dy):
    C = y.shape[1]
    rows = y.numel() // C
    dy = dy.contiguous(memory_format=CL) if y.dim() == 4 else dy.contiguous()
    dx = _empty_like(y)
    kernels().softmax_rows_bwd(dt_code(y.dtype), y.data_ptr(), dy.data_ptr(), dx.data_ptr(), rows, C, stream_ptr())
    return dx


def dropout(x, p, seed, slot=None):
    """Inverted dropout with a Philox mask of (seed, *slot). ``slot``: a 1-element int64 device
    tensor written by :func:`counter_bump` (graph-replay safe: the draw index lives on the device)."""
    y = _empty_like(x)
    kernels().dropout(dt_code(x.dtype), x.data_ptr(), y.data_ptr(), x.numel(), float(p), int(seed) & ((1 << 64) - 1),
                      ptr(slot), stream_ptr())
    return y


def counter_bump(ctr, slot):
    """slot = ++ctr on the device (both 1-element int64 tensors)."""
    kernels().counter_bump(ctr.data_ptr(), slot.data_ptr(), stream_ptr())


def _dp_mask_ok(mask, n, what):
    if mask.dtype != F32 or not mask.is_cuda or mask.numel() != n or not mask.is_contiguous():
        raise ValueError(f"{what}: mask must be a contiguous fp32 GPU tensor of {n} values, got "
                         f"{tuple(mask.shape)} {mask.dtype}")


def drop_path_mask(mask, p, seed, draw=0, slot=None):
    """Write the stochastic-depth mask (droppath.hip) of ``mask.numel()`` samples into ``mask``
    (fp32): 0 with probability p, else 1 / (1 - p), from Philox(seed, draw). ``slot``: a 1-element
    int64 device tensor written by :func:`counter_bump` that holds the draw index instead (graph
    replays then draw a new mask each)."""
    _dp_mask_ok(mask, mask.numel(), "drop_path_mask")
    _rec("drop_path_mask", n=mask.numel())
    kernels().drop_path_mask_into(mask.data_ptr(), mask.numel(), float(p), int(seed) & ((1 << 64) - 1),
                                  int(draw) & ((1 << 64) - 1), ptr(slot), stream_ptr())
    return mask


def drop_path_scale(x, mask, residual=None):
    """y[n] = mask[n] * x[n] (+ residual[n]): the standalone DropPath forward and backward
    (droppath.hip). x: a dense bf16 / fp32 tensor whose samples are contiguous (channels_last 4-D
    or contiguous), at any offset; a dropped sample is written without reading x."""
    if x.dtype not in (F32, BF16) or not x.is_cuda or x.dim() < 1:
        raise ValueError(f"drop_path_scale: expected a bf16 / fp32 GPU tensor, got {tuple(x.shape)} {x.dtype}")
    if not (x.is_contiguous() or (x.dim() == 4 and x.is_contiguous(memory_format=CL))):
        raise ValueError(f"drop_path_scale: x {tuple(x.shape)} strides {tuple(x.stride())} is not dense per sample")
    N = x.shape[0]
    _dp_mask_ok(mask, N, "drop_path_scale")
    if residual is not None and (tuple(residual.shape) != tuple(x.shape) or residual.dtype != x.dtype or not (
            residual.is_contiguous() if x.is_contiguous() else residual.is_contiguous(memory_format=CL))):
        raise ValueError("drop_path_scale: the residual must match x in shape, dtype and layout")
    _rec("drop_path_scale", x=tuple(x.shape), residual=residual is not None)
    # the kernel's 16-byte vectors need x, the residual and the (16-byte aligned) output at the same
    # address modulo 16: a dense view at another offset (batch[k:] of odd rows) is copied first
    if x.data_ptr() % 16:
        x = x.clone(memory_format=torch.preserve_format)
    if residual is not None and residual.data_ptr() % 16:
        residual = residual.clone(memory_format=torch.preserve_format)
    y = _empty_like(x)
    kernels().drop_path_scale(dt_code(x.dtype), x.data_ptr(), mask.data_ptr(), ptr(residual), y.data_ptr(), N,
                              x.numel() // N, stream_ptr())
    return y


def lscale_drop_fwd(x, gamma, mask, residual):
    """The scale tail with stochastic depth (lnorm.hip): y = residual + mask[n] * gamma[c] * x in
    one store; a dropped sample copies its residual rows without reading x."""
    R, C = ln_rows(x, "lscale_drop_fwd")
    assert gamma.dtype == F32 and gamma.numel() == C and gamma.is_contiguous(), "lscale_drop_fwd: gamma fp32 [C]"
    _ln_like(residual, x, "lscale_drop_fwd.residual")
    N = x.shape[0]
    _dp_mask_ok(mask, N, "lscale_drop_fwd")
    _rec("lscale_drop_fwd", x=tuple(x.shape))
    y = _empty_like(x)
    kernels().lscale_drop_fwd(dt_code(x.dtype), x.data_ptr(), gamma.data_ptr(), mask.data_ptr(), residual.data_ptr(),
                              y.data_ptr(), R, C, R // N, stream_ptr())
    return y


def lscale_drop_bwd(dy, x, gamma, mask, dgamma):
    """dx = mask[n] * gamma[c] * dy; dgamma += sum mask[n] * dy * x through the LayerScale's slab
    and fixed-order reduce (bit-reproducible); a dropped sample gets zeros without reading x."""
    R, C = ln_rows(x, "lscale_drop_bwd")
    _ln_like(dy, x, "lscale_drop_bwd.dy")
    for t in (gamma, dgamma):
        assert t.dtype == F32 and t.numel() == C and t.is_contiguous(), "lscale_drop_bwd: gamma / dgamma fp32 [C]"
    N = x.shape[0]
    _dp_mask_ok(mask, N, "lscale_drop_bwd")
    _rec("lscale_drop_bwd", x=tuple(x.shape))
    K = kernels()
    dx = _empty_like(x)
    ws = _empty((K.ln_partial_rows(R, C), C), F32, x.device)
    K.lscale_drop_bwd(dt_code(x.dtype), dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), mask.data_ptr(), dx.data_ptr(),
                      dgamma.data_ptr(), R, C, R // N, ws.data_ptr(), stream_ptr())
    return dx


# ------------------------------------------------------------------------------ loss / optim
LOSS_CODES = {"crossentropy": 0, "softmax_crossentropy": 1, "logsoftmax_crossentropy": 2, "mse": 3, "mae": 4,
              "huber": 5, "soft_crossentropy": 6}


def loss_fused(pred2d, target2d=None, labels=None, kind="softmax_crossentropy", param=1e-15, want_grad=True,
               grad_scale=1.0):
    """Returns (loss[1] f32 device, grad|None, correct[1] int32 device). No host sync. The gradient
    is additionally multiplied by ``grad_scale`` inside the kernel (data parallel: 1 / world)."""
    N, C = pred2d.shape
    pred2d = pred2d.contiguous()
    grad = _empty_like(pred2d) if want_grad else None
    loss = torch.empty((1,), dtype=F32, device=pred2d.device)
    correct = torch.empty((1,), dtype=torch.int32, device=pred2d.device)
    tgt = None
    if target2d is not None:
        tgt = target2d.reshape(N, C).to(F32).contiguous()
    lab = labels.to(torch.int64).contiguous() if labels is not None else None
    K = kernels()
    ws = _empty((K.loss_workspace_floats(N),), F32, pred2d.device) if N > 4 else None
    tk = _ticket(pred2d.device, 0, slot="loss") if N > 4 else None
    K.loss_fused(dt_code(pred2d.dtype), pred2d.data_ptr(), ptr(tgt), ptr(lab), ptr(grad), loss.data_ptr(),
                 correct.data_ptr(), N, C, LOSS_CODES[kind], float(param), float(grad_scale), ptr(ws), ptr(tk),
                 stream_ptr())
    return loss, grad, correct


def mix_batch(x, labels, target, mode, lam, box, num_classes):
    """Mixup / CutMix of the fp32 NCHW device batch ``x`` with its reversed batch, in place, plus the
    dense float32 ``target`` [B, K]: one launch on the current stream, no host sync (mix.hip)."""
    if x.dim() != 4 or x.dtype != F32 or not x.is_cuda or not x.is_contiguous():
        raise ValueError("mix_batch: x is a contiguous float32 GPU [B, C, H, W] tensor")
    B, C, H, W = x.shape
    K = int(num_classes)
    if labels.dtype != torch.int64 or tuple(labels.shape) != (B,) or not labels.is_cuda or not labels.is_contiguous():
        raise ValueError("mix_batch: labels are int64 [B] on the GPU")
    if (K >= 1 and tuple(target.shape) != (B, K)) or target.dtype != F32 or not target.is_cuda \
            or not target.is_contiguous():
        raise ValueError("mix_batch: target is a contiguous float32 GPU [B, num_classes] tensor")
    kernels().mix_batch(x.data_ptr(), labels.data_ptr(), target.data_ptr(), B, C, H, W, int(mode), float(lam),
                        *map(int, box), K, stream_ptr(x.device))
    return x, target


def adam_step(p, g, m, v, shadow, lr, b1, b2, eps, bc1, bc2, wd, decoupled, hyper=None, nodecay=None):
    """One Adam / AdamW step over a flat buffer. ``nodecay`` (uint8 device tensor, one byte per
    64-element block): flagged blocks step with wd = 0 (its own kernel instance; without it the
    launch is the plain adam_kernel)."""
    if nodecay is not None:
        if nodecay.dtype != torch.uint8 or not nodecay.is_cuda or nodecay.numel() * 64 < p.numel():
            raise ValueError("adam_step: nodecay is a uint8 GPU tensor with one entry per 64 elements")
        kernels().adam_step_nodecay(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), ptr(shadow), p.numel(),
                                    float(lr), float(b1), float(b2), float(eps), float(bc1), float(bc2), float(wd),
                                    int(decoupled), ptr(hyper), nodecay.data_ptr(), stream_ptr())
        return
    kernels().adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), ptr(shadow), p.numel(), float(lr),
                        float(b1), float(b2), float(eps), float(bc1), float(bc2), float(wd), int(decoupled),
                        ptr(hyper), stream_ptr())


def sgd_step(p, g, vel, shadow, lr, momentum, hyper=None):
    kernels().sgd_step(p.data_ptr(), g.data_ptr(), ptr(vel), ptr(shadow), p.numel(), float(lr), float(momentum),
                       ptr(hyper), stream_ptr())


def _flat_f32(who, *ts):
    n = ts[0].numel()
    for t in ts:
        if t is not None and (t.dtype != F32 or not t.is_cuda or not t.is_contiguous() or t.numel() != n):
            raise ValueError(f"{who}: flat contiguous float32 GPU buffers of one size")
    return n


def grad_sumsq(g, max_norm, out):
    """``out[4] = {sum g^2, norm, coef, max_norm}`` with ``coef = min(1, max_norm / (norm + 1e-6))``:
    one launch on the current stream, a fixed summation order (bit-reproducible, eager or replayed),
    no host sync. ``out`` is a 4-float device tensor."""
    n = _flat_f32("grad_sumsq", g)
    if out.dtype != F32 or not out.is_cuda or out.numel() < 4 or not out.is_contiguous():
        raise ValueError("grad_sumsq: out is a float32 GPU tensor of 4 elements")
    K = kernels()
    nb = K.grad_sumsq_blocks(n)
    part = _empty((nb,), F32, g.device) if nb > 1 else None
    tk = _ticket(g.device, 0, slot="gradnorm") if nb > 1 else None
    K.grad_sumsq(g.data_ptr(), n, float(max_norm), ptr(part), ptr(tk), out.data_ptr(), stream_ptr(g.device))
    return out


def adam_step_tail(p, g, m, v, shadow, lr, b1, b2, eps, bc1, bc2, wd, decoupled, hyper=None, nodecay=None, coef=None,
                   ema=None, ema_decay=0.0):
    """The Adam / AdamW step with its optional inputs: ``nodecay`` (block table), ``coef`` (a device
    tensor whose first element is the clip coefficient; the step takes ``g * coef``, ``g`` is not
    rewritten) and ``ema`` (``ema = d ema + (1 - d) p_new``). Launched only when clip or EMA is on."""
    n = _flat_f32("adam_step_tail", p, g, m, v, ema)
    if nodecay is not None and (nodecay.dtype != torch.uint8 or not nodecay.is_cuda or nodecay.numel() * 64 < n):
        raise ValueError("adam_step_tail: nodecay is a uint8 GPU tensor with one entry per 64 elements")
    kernels().adam_step_tail(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), ptr(shadow), n, float(lr),
                             float(b1), float(b2), float(eps), float(bc1), float(bc2), float(wd), int(decoupled),
                             ptr(hyper), ptr(nodecay), ptr(coef), ptr(ema), float(ema_decay), stream_ptr(p.device))


def sgd_step_tail(p, g, vel, shadow, lr, momentum, hyper=None, coef=None, ema=None, ema_decay=0.0):
    n = _flat_f32("sgd_step_tail", p, g, vel, ema)
    kernels().sgd_step_tail(p.data_ptr(), g.data_ptr(), ptr(vel), ptr(shadow), n, float(lr), float(momentum),
                            ptr(hyper), ptr(coef), ptr(ema), float(ema_decay), stream_ptr(p.device))


def layerwise_workspace(tables, device):
    """``(trust, part)`` for :func:`lamb_step` / :func:`lars_step`: the trust table (``[3 * nsegs]``:
    trust, then the pairs ``{sum p^2, sum u^2}``) and the per-chunk partial pairs (``[2 * nchunks]``)."""
    return (torch.ones(max(3 * tables.nsegs, 1), dtype=F32, device=device),
            torch.zeros(max(2 * tables.nchunks, 1), dtype=F32, device=device))


def _layerwise_args(who, n, tables, trust, part, device):
    if tables.chunks_dev is None or tables.chunks_dev.device != device:
        raise ValueError(f"{who}: the segment tables live on {tables.device}, the buffers on {device}")
    if tables.cover > n:
        raise ValueError(f"{who}: the chunk table reaches element {tables.cover}, the buffers hold {n} "
                         f"(chunks are whole 64-element blocks inside the buffers)")
    for name, t, need in (("trust", trust, 3 * tables.nsegs), ("part", part, 2 * tables.nchunks)):
        if t.dtype != F32 or not t.is_cuda or not t.is_contiguous() or t.numel() < need:
            raise ValueError(f"{who}: {name} is a float32 GPU tensor of at least {need} elements")
    tk = _ticket(device, 0, slot="layerwise")
    return (tables.chunks_dev.data_ptr(), tables.nchunks, tables.segs_dev.data_ptr(), tables.nsegs, tables.cover,
            part.data_ptr(), tk.data_ptr(), trust.data_ptr(), stream_ptr(device))


def lamb_step(p, g, m, v, shadow, lr, b1, b2, eps, bc1, bc2, wd, tables, trust, part, hyper=None, coef=None,
              ema=None, ema_decay=0.0):
    """One LAMB step over a flat buffer: two launches on the current stream, no host sync, a fixed
    summation order (bit-reproducible, eager or replayed). ``tables``: :class:`SegmentTables` on the
    buffers' device; ``trust`` / ``part``: :func:`layerwise_workspace`. ``hyper`` (device ``{lr, bc1,
    bc2}``), ``coef`` and ``ema`` are optional as in :func:`adam_step_tail`."""
    n = _flat_f32("lamb_step", p, g, m, v, ema)
    kernels().lamb_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), ptr(shadow), n, float(lr), float(b1),
                        float(b2), float(eps), float(bc1), float(bc2), float(wd), ptr(hyper), ptr(coef), ptr(ema),
                        float(ema_decay), *_layerwise_args("lamb_step", n, tables, trust, part, p.device))


def lars_step(p, g, vel, shadow, lr, momentum, wd, trust_coefficient, eps, tables, trust, part, hyper=None,
              coef=None, ema=None, ema_decay=0.0):
    """One LARS step over a flat buffer (``vel`` None: no momentum); see :func:`lamb_step`. ``hyper``
    is the device ``{lr}``."""
    n = _flat_f32("lars_step", p, g, vel, ema)
    kernels().lars_step(p.data_ptr(), g.data_ptr(), ptr(vel), ptr(shadow), n, float(lr), float(momentum), float(wd),
                        float(trust_coefficient), float(eps), ptr(hyper), ptr(coef), ptr(ema), float(ema_decay),
                        *_layerwise_args("lars_step", n, tables, trust, part, p.device))


def ema_swap(a, b, shadow=None):
    """Exchange two flat fp32 buffers in one launch; ``shadow`` (bf16, optional) is refreshed from the
    new ``a``. Twice restores every bit."""
    n = _flat_f32("ema_swap", a, b)
    if shadow is not None and shadow.numel() != n:
        raise ValueError("ema_swap: the shadow has the buffers' size")
    kernels().ema_swap(a.data_ptr(), b.data_ptr(), ptr(shadow), n, stream_ptr(a.device))


def zero_(t):
    """Zero a dense GPU tensor on the current stream with the library's own fill kernel (no ATen
    fill on the hot path). Not hipMemsetAsync: captured into a hipGraph, a memset node wrote
    garbage from its second replay on (ROCm 7.2; observed with a capture of two memset nodes)."""
    assert t.is_cuda and (t.is_contiguous() or t.is_contiguous(memory_format=CL))
    kernels().zero_bytes(t.data_ptr(), t.numel() * t.element_size(), stream_ptr(t.device))
    return t


def cast_bf16(src, dst):
    kernels().cast_f32_bf16(src.data_ptr(), dst.data_ptr(), src.numel(), stream_ptr())


class WeightTransposer:
    """Regenerates every conv's dgrad operand ([Ci][KH][KW][Co]) from the bf16 shadow weights (or,
    on the fp32 compute path, the fp32 channels_last masters) in ONE kernel launch per step
    (instead of one launch per conv)."""

    def __init__(self, convs, dtype=BF16):
        self.dtype = dtype
        self.convs = [c for c in convs if c.in_channels % 8 == 0 and c.out_channels % 8 == 0]
        rows = []
        self.max_tiles = 0  # 64x64 (co, ci) tiles per tap: the launch's x extent
        for c in self.convs:
            w = c.weight_operand(0)
            Co, Ci, KH, KW = w.shape
            assert w.dtype == dtype and (w.is_contiguous(memory_format=CL) or KH * KW == 1)
            c._wt_buf = _arena.persistent((Ci, KH, KW, Co), dtype, w.device)
            rows.append([w.data_ptr(), c._wt_buf.data_ptr(), Co, KH * KW, Ci])
            self.max_tiles = max(self.max_tiles, KH * KW * ((Co + 63) // 64) * ((Ci + 63) // 64))
        self.table = torch.tensor(rows, dtype=torch.int64).to(self.convs[0]._wt_buf.device) if rows else None

    def run(self):
        if self.table is None:
            return
        kernels().multi_weight_transpose(self.table.data_ptr(), len(self.convs), self.max_tiles, stream_ptr(),
                                         int(self.dtype == F32))
        for c in self.convs:
            c._wt_valid = True

    def invalidate(self):
        for c in self.convs:
            c._wt_valid = False


def im2col(x, kh, kw, sh, sw, ph, pw):
    N, C, H, W = x.shape
    OH, OW = conv_out_hw(H, W, kh, kw, sh, sw, ph, pw)
    x = x.contiguous().float()
    col = _empty((C * kh * kw, N * OH * OW), F32, x.device)
    kernels().im2col(x.data_ptr(), col.data_ptr(), N, C, H, W, kh, kw, sh, sw, ph, pw, OH, OW, stream_ptr())
    return col


def col2im(col, x_shape, kh, kw, sh, sw, ph, pw):
    N, C, H, W = x_shape
    OH, OW = conv_out_hw(H, W, kh, kw, sh, sw, ph, pw)
    x = _empty((N, C, H, W), F32, col.device)
    kernels().col2im(col.contiguous().data_ptr(), x.data_ptr(), N, C, H, W, kh, kw, sh, sw, ph, pw, OH, OW,
                     stream_ptr())
    return x
