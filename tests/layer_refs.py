"""Plain-torch references of the generic layer kernels (GroupNorm, average pool, activations, row
softmax, the six loss kinds 0..5), the shared tolerance rules and the case lists of the tests that use
them: tests/test_layer_refs_cpu.py checks the references themselves (torch autograd and the native CPU
backend, float64) and tests/test_gpu_layer_kernels.py compares the HIP kernels with them.

Every reference computes in the dtype of the floating-point tensors it is given, so the same code
gives the float64 reference and, through :func:`noise_floor`, its own float32 error. A reference takes
the already-rounded inputs: a bf16 case rounds its inputs to bf16 first (:func:`rounded`) and evaluates
in float64. Nothing here touches a GPU.

Tolerances (elementwise, ``ref`` in float64):

* fp32 results: ``|got - ref| <= 8 e32 + 2^-20 max|ref|`` with ``e32 = noise_floor(reference,
  inputs)``: the float32-against-float64 error of the reference itself, times 8 because a kernel's
  tree summation order is not the reference's; the second term is eight float32 ulps of the largest
  result (a result the reference happens to get exactly in float32 still gets that much).
* bf16 results: the kernel computes in fp32 and rounds once: one bf16 ulp of the result (2^-8 |ref|)
  on top of the fp32 rule. The fp32 outputs of a bf16 run (statistics, parameter gradients, the loss)
  use the fp32 rule.
* activations and softmax use the fast ``__expf``, whose error e32 does not capture: the bound of
  tests/test_gpu_kernels.py::test_pools_and_act, 1e-5 relative, applied elementwise with an absolute
  floor of 1e-6 (plus the bf16 ulp for bf16).
"""
import math

import torch

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
CL = torch.channels_last

# ------------------------------------------------------------------------------ case lists
# (N, C, G, H, W)
GN_CASES = [(2, 8, 8, 5, 3),      # Cg = 1
            (3, 12, 1, 4, 4),     # G = 1
            (2, 24, 4, 7, 5),     # Cg = 6
            (1, 4, 2, 1, 1),      # 2 elements per group
            (2, 32, 4, 9, 9),     # 648 elements per group: not a multiple of the 256 threads
            (1, 640, 2, 2, 2),    # Cg = 320 > 256: the stride loop of the affine partials
            (5, 16, 4, 3, 3)]     # general
GN_LARGE_MEAN = (2, 32, 4, 9, 9)
GN_EPS = 1e-5

# (N, C, H, W, ph, pw, sh, sw, pdh, pdw)
POOL_CASES = [(2, 12, 7, 9, 3, 3, 2, 2, 1, 1),   # padding, overlapping windows
              (1, 3, 5, 5, 3, 3, 1, 1, 1, 1),    # padding, stride 1
              (2, 8, 6, 8, 2, 3, 2, 3, 0, 0),    # non-square window
              (2, 16, 9, 9, 2, 2, 3, 3, 0, 0),   # stride > window: inputs without a gradient
              (3, 40, 4, 4, 4, 4, 4, 4, 0, 0),   # global kernels
              (2, 64, 7, 7, 7, 7, 1, 1, 0, 0),   # global kernels
              (1, 8, 1, 1, 1, 1, 1, 1, 0, 0)]    # identity
POOL_GLOBAL = (POOL_CASES[4], POOL_CASES[5])

ACT_KINDS = ["relu", "leaky_relu", "elu", "sigmoid", "tanh", "linear", "gelu"]
ACT_NS = [1, 7, 8, 9, 1003]
ACT_ALPHAS = {"leaky_relu": (0.01, 0.2), "elu": (1.0, 0.5)}
ACT_KINK = 1e-3  # no input but the deliberate 0.0 lies this close to the kink at 0
ACT_SATURATING = [20.0, -20.0, 88.0, -88.0, 1e-30, -1e-30]

# (rows, C): every rows value of {1, 3, 5, 257} and every C of {1, 10, 63, 64, 65, 200, 1000} at least
# once, a partly filled last workgroup (rows % 4 != 0) on both sides of the 64-lane stride
SOFTMAX_CASES = [(5, 65), (257, 10), (1, 1000), (3, 1), (1, 63), (3, 64), (5, 200), (257, 1), (3, 1000), (1, 10),
                 (5, 64), (257, 63)]
SOFTMAX_4D = (2, 10, 3, 3)

LOSS_KINDS = ["crossentropy", "softmax_crossentropy", "logsoftmax_crossentropy", "mse", "mae", "huber"]
LOSS_SHAPES = [(1, 10), (3, 65), (4, 64), (5, 63), (7, 200), (257, 10), (1025, 2)]
LOSS_PARAM = {"crossentropy": 2.0 ** -10, "huber": 0.5}  # exact in float32, as the kernel receives them
LOSS_KINK = 1e-3  # |d| and |d - param| stay this far from the MAE / Huber kinks
# rows with equal maxima: (C, the classes that share the maximum)
TIE_SETS = [(10, (3, 7)), (65, (3, 64)), (10, (5, 6)), (200, (70, 130, 190)), (200, (3, 67)), (200, (5, 6))]


# ------------------------------------------------------------------------------ helpers
def rounded(t, dtype):
    """t rounded to ``dtype`` (bf16 or fp32), as the float32 tensor holding those values."""
    return t.to(dtype).float()


def _cast(v, dtype):
    return v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v


def evaluate(fn, dtype, *inputs):
    """fn on the inputs with every floating-point tensor cast to ``dtype``; a tuple of tensors."""
    out = fn(*[_cast(v, dtype) for v in inputs])
    return out if isinstance(out, tuple) else (out,)


def noise_floor(fn, *inputs):
    """The reference's own float32 error: per output of ``fn``, the max-abs difference between fn
    evaluated in float32 and in float64 on the same inputs. Never involves a kernel."""
    lo, hi = evaluate(fn, F32, *inputs), evaluate(fn, F64, *inputs)
    return tuple(float((a.double() - b.double()).abs().max()) if b.numel() else 0.0 for a, b in zip(lo, hi))


def tol32(ref, e32):
    """Elementwise bound of an fp32 result (a float): 8 e32 + 2^-20 max|ref|."""
    return 8.0 * e32 + 2.0 ** -20 * float(ref.abs().max())


def tol_bf16(ref, e32):
    """Elementwise bound of a bf16 result (a tensor): one bf16 ulp of the result plus the fp32 rule."""
    return 2.0 ** -8 * ref.abs() + tol32(ref, e32)


def tol_fast(ref, bf16):
    """Elementwise bound of the ``__expf`` kernels (activations, softmax): 1e-5 relative, 1e-6 absolute."""
    t = 1e-5 * ref.abs() + 1e-6
    return t + 2.0 ** -8 * ref.abs() if bf16 else t


def worst(got, ref, tol):
    """(max |got - ref|, max of |got - ref| / tol) in float64 on the CPU."""
    ref = ref.double()
    err = (got.detach().double().cpu().reshape(ref.shape) - ref).abs()
    if err.numel() == 0:
        return 0.0, 0.0
    t = tol if torch.is_tensor(tol) else torch.full_like(err, float(tol))
    return float(err.max()), float((err / t.clamp_min(1e-300)).max())


# ------------------------------------------------------------------------------ GroupNorm
def gn_fwd(x, G, gamma, beta, eps=GN_EPS):
    """(y, mean [N G], istd [N G]) of x [N, C, H, W]; biased variance about the mean (two passes)."""
    N, C, H, W = x.shape
    xg = x.reshape(N, G, -1)
    mean = xg.mean(2)
    d = xg - mean[:, :, None]
    var = (d * d).mean(2)
    istd = 1.0 / torch.sqrt(var + eps)
    y = (d * istd[:, :, None]).reshape(N, C, H, W)
    if gamma is not None:
        y = y * gamma.view(1, C, 1, 1)
    if beta is not None:
        y = y + beta.view(1, C, 1, 1)
    return y, mean.reshape(-1), istd.reshape(-1)


def gn_var(x, G):
    """Biased per-(image, group) variance [N G]."""
    xg = x.reshape(x.shape[0], G, -1)
    d = xg - xg.mean(2, keepdim=True)
    return (d * d).mean(2).reshape(-1)


def gn_bwd(x, dy, G, gamma, eps=GN_EPS):
    """(dx, dgamma, dbeta) of :func:`gn_fwd` (the statistics are recomputed from x)."""
    N, C, H, W = x.shape
    _, mean, istd = gn_fwd(x, G, None, None, eps)
    mu, is_ = mean.view(N, G, 1), istd.view(N, G, 1)
    xh = (x.reshape(N, G, -1) - mu) * is_
    d = dy if gamma is None else dy * gamma.view(1, C, 1, 1)
    d = d.reshape(N, G, -1)
    m1 = d.mean(2, keepdim=True)
    m2 = (d * xh).mean(2, keepdim=True)
    dx = (is_ * (d - m1 - xh * m2)).reshape(N, C, H, W)
    xh4 = xh.reshape(N, C, H, W)
    return dx, (dy * xh4).sum((0, 2, 3)), dy.sum((0, 2, 3))


# ------------------------------------------------------------------------------ average pool
def pool_out(H, W, ph, pw, sh, sw, pdh, pdw):
    return (H + 2 * pdh - ph) // sh + 1, (W + 2 * pdw - pw) // sw + 1


def avgpool_fwd(x, ph, pw, sh, sw, pdh, pdw):
    """count_include_pad: every window is divided by ph pw, the padding counts as zeros."""
    N, C, H, W = x.shape
    OH, OW = pool_out(H, W, ph, pw, sh, sw, pdh, pdw)
    xp = x.new_zeros(N, C, H + 2 * pdh, W + 2 * pdw)
    xp[:, :, pdh:pdh + H, pdw:pdw + W] = x
    y = x.new_zeros(N, C, OH, OW)
    for ky in range(ph):
        for kx in range(pw):
            y = y + xp[:, :, ky:ky + (OH - 1) * sh + 1:sh, kx:kx + (OW - 1) * sw + 1:sw]
    return y / (ph * pw)


def avgpool_bwd(dy, H, W, ph, pw, sh, sw, pdh, pdw):
    N, C, OH, OW = dy.shape
    dxp = dy.new_zeros(N, C, H + 2 * pdh, W + 2 * pdw)
    for ky in range(ph):
        for kx in range(pw):
            dxp[:, :, ky:ky + (OH - 1) * sh + 1:sh, kx:kx + (OW - 1) * sw + 1:sw] += dy
    return dxp[:, :, pdh:pdh + H, pdw:pdw + W] / (ph * pw)


def distinct_dy(N, C, dtype):
    """A global pool's dy [N, C, 1, 1]: a distinct value per (n, c), each exact in bf16, in a scrambled
    order so that neither a swapped nor a dropped index reproduces it."""
    assert N * C <= 128
    k = (torch.arange(N * C) * 37) % 128  # 37 is odd: a permutation of 0..127
    return rounded((k.float() - 63.5) / 16.0, dtype).view(N, C, 1, 1)


# ------------------------------------------------------------------------------ activations
def act_fwd(x, kind, alpha=0.0):
    if kind == "relu":
        return torch.where(x > 0, x, torch.zeros_like(x))
    if kind == "leaky_relu":
        return torch.where(x > 0, x, alpha * x)
    if kind == "elu":
        return torch.where(x > 0, x, alpha * (torch.exp(x) - 1.0))
    if kind == "sigmoid":
        return 1.0 / (1.0 + torch.exp(-x))
    if kind == "tanh":
        return torch.tanh(x)
    if kind == "gelu":  # the exact form x Phi(x)
        return 0.5 * x * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))
    assert kind == "linear"
    return x.clone()


def act_grad(x, kind, alpha=0.0):
    """The derivative at x (the backward is dy times this); at 0 the one-sided value for x <= 0."""
    one, zero = torch.ones_like(x), torch.zeros_like(x)
    if kind == "relu":
        return torch.where(x > 0, one, zero)
    if kind == "leaky_relu":
        return torch.where(x > 0, one, alpha * one)
    if kind == "elu":
        return torch.where(x > 0, one, alpha * torch.exp(x))
    if kind == "sigmoid":
        s = 1.0 / (1.0 + torch.exp(-x))
        return s * (1.0 - s)
    if kind == "tanh":
        t = torch.tanh(x)
        return 1.0 - t * t
    if kind == "gelu":  # Phi(x) + x phi(x)
        return 0.5 * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0)))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    assert kind == "linear"
    return one


def act_alphas(kind):
    return ACT_ALPHAS.get(kind, (0.0,))


def act_inputs(n, dtype, seed=0):
    """(x, dy) of n values rounded to ``dtype``: x in [-10, 10] with an exact 0.0 in the middle and no
    other value within ACT_KINK of 0."""
    g = torch.Generator().manual_seed(1000 * n + seed)
    x = torch.rand(n, generator=g) * 20.0 - 10.0
    x = torch.where(x.abs() < 4 * ACT_KINK, x + 0.5, x)
    x = rounded(x, dtype)
    x[n // 2] = 0.0
    dy = rounded(torch.randn(n, generator=g), dtype)
    return x, dy


# ------------------------------------------------------------------------------ softmax
def softmax_fwd(x):
    """softmax over dim 1."""
    e = torch.exp(x - x.max(1, keepdim=True).values)
    return e / e.sum(1, keepdim=True)


def softmax_bwd(y, dy):
    return y * (dy - (y * dy).sum(1, keepdim=True))


# ------------------------------------------------------------------------------ losses
def one_hot(labels, C, dtype=F32):
    t = torch.zeros(labels.numel(), C, dtype=dtype)
    t[torch.arange(labels.numel()), labels] = 1.0
    return t


def first_argmax(v):
    """Row arg-max of a 2-D tensor, the lowest index among equal maxima."""
    C = v.shape[1]
    idx = torch.arange(C).expand_as(v)
    return torch.where(v == v.max(1, keepdim=True).values, idx, torch.full_like(idx, C)).min(1).values


def loss_ref(pred, target, kind, param=0.0, grad_scale=1.0):
    """(loss [1], grad [N, C], correct [1] int64) of a dense target [N, C], the rules of loss_row:
    the loss term of a row uses its first class with target > 0.5, and a row without one adds no loss
    but still gets its gradient; ``correct`` counts the rows whose first-maximum arg-max of prediction
    and target agree; crossentropy clamps the probability to [param, 1 - param]; mse / mae / huber
    are scaled by 1 / (N C), the cross entropies by 1 / N."""
    N, C = pred.shape
    t = target.to(pred.dtype)
    correct = (first_argmax(pred) == first_argmax(t)).sum().reshape(1)
    idx = torch.arange(C).expand(N, C)
    hot = torch.where(t > 0.5, idx, torch.full_like(idx, C)).min(1).values
    has = hot < C
    hotc = hot.clamp(max=C - 1).view(N, 1)
    if kind in ("softmax_crossentropy", "logsoftmax_crossentropy"):
        m = pred.max(1, keepdim=True).values
        e = torch.exp(pred - m)
        s = e.sum(1, keepdim=True)
        lse = (m + torch.log(s)).view(N)
        rows = torch.where(has, lse - pred.gather(1, hotc).view(N), torch.zeros_like(lse))
        return rows.sum().reshape(1) / N, (e / s - t) * (grad_scale / N), correct
    if kind == "crossentropy":
        v = pred.gather(1, hotc).view(N).clamp(param, 1.0 - param)
        rows = torch.where(has, -torch.log(v), torch.zeros_like(v))
        return rows.sum().reshape(1) / N, (pred - t) * (grad_scale / N), correct
    d = pred - t
    sign = torch.where(d > 0, torch.ones_like(d), -torch.ones_like(d))
    if kind == "mse":
        l, g = d * d, 2.0 * d
    elif kind == "mae":
        l, g = d.abs(), sign
    else:
        assert kind == "huber"
        small = d.abs() <= param
        l = torch.where(small, 0.5 * d * d, param * d.abs() - 0.5 * param * param)
        g = torch.where(small, d, param * sign)
    return l.sum().reshape(1) / (N * C), g * (grad_scale / (N * C)), correct


def loss_case(kind, N, C, dtype, soft=False, seed=0):
    """(pred, labels, dense target, param) of one loss case, the prediction rounded to ``dtype``.

    Every row has a clear arg-max (ties have cases of their own); about half of the rows are hits.
    crossentropy: softmax outputs, the hot class of row 0 pushed below ``param`` (the clamp's lower
    side); mae / huber: |pred - target| kept LOSS_KINK away from 0 and from ``param``, on both sides
    of ``param``. The target is the one-hot form of the labels, or with ``soft`` its
    :func:`soft_rows` (same predictions for the cross entropies)."""
    g = torch.Generator().manual_seed(7919 * N + 31 * C + seed)
    param = LOSS_PARAM.get(kind, 0.0)
    lab = torch.randint(0, C, (N,), generator=g)
    win = torch.randint(0, C, (N,), generator=g)
    win[::2] = lab[::2]
    r = torch.arange(N)
    t = soft_rows(one_hot(lab, C)) if soft else one_hot(lab, C)
    if kind in ("mse", "mae", "huber"):
        # |d| in (0.05, 0.3), below param, or in (0.6, 1.1), above it: the bf16 rounding of a prediction
        # below 4 moves it by at most 2^-7, which leaves both margins
        mag = 0.05 + torch.rand(N, C, generator=g) * 0.25
        big = torch.rand(N, C, generator=g) < 0.5
        mag = torch.where(big, 0.6 + torch.rand(N, C, generator=g) * 0.5, mag)
        sgn = torch.where(torch.rand(N, C, generator=g) < 0.5, -1.0, 1.0)
        x = t + sgn * mag
        x[r, win] = 2.5 + torch.rand(N, generator=g) * 0.25  # the clear arg-max: d >= 1.5
    else:
        x = 3.0 * torch.randn(N, C, generator=g)
        x[r, win] = x.max(1).values + 1.0
        if kind == "crossentropy":
            x = torch.softmax(x.double(), 1).float()
            x[0, lab[0]] = param / 4  # the hot class of row 0 lies below the clamp
    return rounded(x, dtype), lab, t, param


def soft_rows(t):
    """t with every third row (from row 1) replaced by a row whose entries are all <= 0.5: no class
    qualifies for the loss term, the gradient is still written."""
    t = t.clone()
    C = t.shape[1]
    for n in range(1, t.shape[0], 3):
        k = int(t[n].argmax())
        t[n] = 0.0
        t[n, k] = 0.5
        t[n, (k + 1) % C] += 0.25
    return t


def tied_target_case(C, ties, dtype, N=7):
    """(pred, dense target) of N rows whose *target* maximum (0.5) is shared by the classes ``ties``;
    the prediction has a clear arg-max, ties[0] in the first four rows and the remaining tied classes
    in turn after that: the first-index rule on the target counts exactly 4 hits, any other fewer."""
    g = torch.Generator().manual_seed(193 * C + sum(ties))
    x = torch.randn(N, C, generator=g)
    rest = ties[1:]
    win = torch.tensor([ties[0]] * 4 + [rest[n % len(rest)] for n in range(N - 4)])
    x[torch.arange(N), win] = x.max(1).values + 1.0
    t = torch.rand(N, C, generator=g) * 0.25
    for k in ties:
        t[:, k] = 0.5
    return rounded(x, dtype), t


def tie_case(C, ties, dtype, N=7):
    """(pred, labels) of N rows whose maximum is shared by the classes ``ties`` (exactly equal values
    after the rounding). The first four rows are labelled ties[0] and the others take the remaining
    classes in turn, so the first-index rule counts exactly 4 hits and a rule that picks any other of
    the tied classes counts fewer."""
    g = torch.Generator().manual_seed(97 * C + sum(ties))
    x = rounded(torch.randn(N, C, generator=g), dtype)
    top = rounded(x.max(1).values + 1.0, dtype)
    for k in ties:
        x[:, k] = top
    rest = ties[1:]
    lab = torch.tensor([ties[0]] * 4 + [rest[n % len(rest)] for n in range(N - 4)], dtype=torch.int64)
    return x, lab
