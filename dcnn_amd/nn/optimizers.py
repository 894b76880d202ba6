"""Optimizers (reference `include/nn/optimizers.hpp:25-306`): SGD(+momentum), Adam, AdamW, and the
layer-wise adaptive LAMB and LARS (``_Layerwise``: a trust ratio per parameter, two launches a step).

``attach(params, grads)`` as in the reference. When the attached tensors are exactly the views
of one :class:`ParamArena` (the normal case: a Sequential or a pipeline stage), the update is
ONE fused kernel over the flat buffer which also refreshes the bf16 shadow weights. The step
scalars live in a tiny device tensor ``{lr, bc1, bc2, t}``: Adam's step counter and bias
corrections advance ON THE DEVICE (``adam_scalars``, captured in the step graph ahead of the
update), and the learning rate is uploaded only when it changes — a replayed training step needs
no host-to-device transfer besides its input batch. A CPU arena is updated by the native
backend's flat-buffer loops (``ops/cpu.py``), in the arena's dtype (float32 or float64).

Every optimizer takes two switches that belong to the step, both off by default:

``max_grad_norm > 0``: global-norm gradient clipping (torch's ``clip_grad_norm_``, L2). One
deterministic reduction over the flat gradient leaves ``{sumsq, norm, coef, max_norm}`` with
``coef = min(1, max_grad_norm / (norm + 1e-6))`` in device memory (``opt.grad_norm_device``) and the
step takes ``g * coef``: no host read, so a captured step stays one graph. The gradient buffers are
NOT rewritten: ``model.gradients()`` still shows the unclipped gradient. A non-finite norm propagates
into the step as it does in torch; no step is skipped. Under data parallelism the norm is taken when
the step is launched, behind the all-reduce: it is the norm of the averaged gradient.

``ema_decay`` in (0, 1): an exponential moving average of the weights, ``opt.ema`` (a flat fp32
buffer of the arena's size, a copy of the weights at ``attach``), updated inside the step kernel:
``ema = d ema + (1 - d) p_new`` with a fixed decay (no warm-up of the decay). BatchNorm running
statistics are not averaged: evaluating inside ``opt.ema_weights()`` uses the live statistics.

With both off a step launches exactly what it launched before they existed.
"""
from __future__ import annotations

import contextlib
import inspect
import math
from typing import List, Optional

import torch


class OptimizerConfig(dict):
    def __init__(self, type: str, name: str = "", parameters: Optional[dict] = None):
        super().__init__(type=type, name=name, parameters=dict(parameters or {}))

    @property
    def type(self):
        return self["type"]

    def to_json(self):
        return dict(self)

    @staticmethod
    def from_json(j):
        return OptimizerConfig(j.get("type", ""), j.get("name", ""), j.get("parameters", {}))


def _arena_of(params: List[torch.Tensor]):
    """Return the ParamArena if params are exactly its views in order (fused flat path)."""
    if not params:
        return None
    base = params[0]._base if params[0]._base is not None else None
    if base is None:
        return None
    for p in params:
        if p._base is None or p._base.data_ptr() != base.data_ptr():
            return None
    return base


def _check_tail(max_grad_norm, ema_decay):
    mg, ed = float(max_grad_norm), float(ema_decay)
    if not mg >= 0.0 or math.isinf(mg):
        raise ValueError(f"max_grad_norm {max_grad_norm!r} is not a finite value >= 0 (0 switches clipping off)")
    if not 0.0 <= ed < 1.0:
        raise ValueError(f"ema_decay {ema_decay!r} is not in [0, 1) (0 switches the weight EMA off)")
    return mg, ed


def refuse_tail_options(config, who: str) -> None:
    """Raise for an optimizer config with clipping or the weight EMA on, where they cannot be honoured
    (a pipeline stage: its norm is not the model's norm, and the flat optimizer-state transfer does not
    know the EMA buffer)."""
    params = (config or {}).get("parameters", {}) if isinstance(config, dict) else {}
    for key in ("max_grad_norm", "ema_decay"):
        if float(params.get(key, 0.0) or 0.0) != 0.0:
            raise ValueError(f"{who}: optimizer option {key}={params[key]!r} is not supported on a pipeline "
                             f"stage (a per-stage gradient norm is not the model's norm, and the stage's "
                             f"optimizer-state transfer does not carry an EMA buffer)")


class Optimizer:
    def __init__(self, learning_rate: float, max_grad_norm: float = 0.0, ema_decay: float = 0.0):
        self.learning_rate = float(learning_rate)
        self.max_grad_norm, self.ema_decay = _check_tail(max_grad_norm, ema_decay)
        self.ema: Optional[List[torch.Tensor]] = None  # [flat buffer] on an arena, else one per parameter
        self.grad_norm_device: Optional[torch.Tensor] = None  # {sumsq, norm, coef, max_norm}
        self._model = None
        self.params: List[torch.Tensor] = []
        self.grads: List[torch.Tensor] = []
        self.arena = None
        self.no_decay: Optional[List[bool]] = None
        self._flat_p = self._flat_g = None
        self._hyper = None
        self._hyper_dirty = True  # device scalars must be (re)uploaded before the next step

    def attach(self, params, grads=None, arena=None, no_decay=None) -> None:
        """``no_decay``: one bool per parameter, True for those excluded from weight decay (biases,
        norm affines, layer scales — each layer classes its own, ``ParamSpec.no_decay``). Taken
        from the model or the arena when one is given."""
        self._model = None
        if grads is None and hasattr(params, "parameters"):
            model = self._model = params
            params, grads = model.parameters(), model.gradients()
            arena = getattr(model, "arena", None)
            if no_decay is None and hasattr(model, "no_decay_flags"):
                no_decay = model.no_decay_flags()
        self.params, self.grads = list(params), list(grads)
        if len(self.params) != len(self.grads):
            raise ValueError("params/grads length mismatch")
        if no_decay is None and arena is not None and len(arena.specs) == len(self.params):
            no_decay = arena.no_decay_flags()
        if no_decay is not None and len(no_decay) != len(self.params):
            raise ValueError("params/no_decay length mismatch")
        self.no_decay = None if no_decay is None else [bool(f) for f in no_decay]
        self.arena = arena
        if self.arena is not None:
            ptrs = [p.data_ptr() for p in self.params]
            own = [self.arena.param(i).data_ptr() for i in range(len(self.arena.specs))]
            if ptrs != own:
                self.arena = None
        if self.arena is not None:
            self._flat_p, self._flat_g = self.arena.data, self.arena.grad
        # re-attaching resets the step state (Adam t, m, v): the device scalars (step counter,
        # learning rate) must be re-uploaded too, or the device keeps counting from the old t
        self._hyper_dirty = True
        self._on_attach()
        self._attach_tail()

    def _on_attach(self):
        pass

    def _need_no_decay_flags(self):
        if self.no_decay_norm_bias and self.no_decay is None:
            raise ValueError("no_decay_norm_bias needs to know which parameters are biases, norm affines or "
                             "layer scales: attach a model or an arena, or pass no_decay=[...]")

    def fused(self) -> bool:
        """The step is the fused launch over a GPU arena's flat buffers."""
        return self.arena is not None and self._flat_p.is_cuda

    def prepare_step(self) -> None:
        """Host side of a step (graph-replay safe): host counters, and the device scalars when stale."""

    def launch_step(self) -> None:
        """Device side of a fused step: the launches, reading their scalars from device memory."""
        raise NotImplementedError

    def _step_cpu_arena(self, cpu) -> None:
        """The native flat-buffer step over a CPU arena (``cpu``: ``ops.cpu``; float32 or float64)."""
        raise NotImplementedError

    def _step_param(self, i, p, g) -> None:
        """Parameter ``i`` in torch, under ``no_grad``; ``g`` is already scaled by the clip coefficient."""
        raise NotImplementedError

    def update(self) -> None:
        """One step: fused over a GPU arena, the native flat-buffer loops over a CPU arena (then the
        shadow refresh), else parameter by parameter in torch with the EMA behind each."""
        self.prepare_step()
        if self.fused():
            self.launch_step()
        elif self.arena is not None:
            from ..ops import cpu
            self._step_cpu_arena(cpu)
            self.arena.sync_shadow()
        else:
            coef = self._host_coef()  # over all parameters, before any of them is stepped
            with torch.no_grad():
                for i, (p, g) in enumerate(zip(self.params, self.grads)):
                    self._step_param(i, p, g if coef is None else g * coef)
                    self._ema_torch(i, p)

    step = property(lambda self: self.update)

    # ------------------------------------------------------------ gradient clipping / weight EMA
    def _tail(self) -> bool:
        return self.max_grad_norm > 0.0 or self.ema_decay > 0.0

    def _attach_tail(self):
        self.ema = self.grad_norm_device = None
        if not self.params:
            return
        if self.ema_decay > 0.0:
            if self.arena is not None:
                self.ema = [self.arena.new_zeros()]
                self.ema[0].copy_(self.arena.data)
            else:
                self.ema = [p.detach().clone() for p in self.params]
        if self.max_grad_norm > 0.0:
            ref = self._flat_p if self.arena is not None else self.params[0]
            self.grad_norm_device = torch.zeros(4, dtype=ref.dtype, device=ref.device)
            self.grad_norm_device[2] = 1.0
            self.grad_norm_device[3] = self.max_grad_norm

    def _launch_norm(self):
        """GPU arena: the norm of the gradient the step is about to consume, left on the device."""
        if self.max_grad_norm > 0.0:
            from ..ops import hip
            hip.grad_sumsq(self._flat_g, self.max_grad_norm, self.grad_norm_device)
            return self.grad_norm_device[2:3]
        return None

    def _host_coef(self):
        """CPU paths: the global norm over ALL gradients (not per tensor) and the coefficient, also
        written to ``grad_norm_device``. None when clipping is off."""
        if not self.max_grad_norm > 0.0:
            return None
        if self.arena is not None:
            from ..ops import cpu
            sumsq = cpu.grad_sumsq(self._flat_g)
        else:
            sumsq = float(sum(float((g.detach().double() ** 2).sum()) for g in self.grads))
        norm = math.sqrt(sumsq) if sumsq == sumsq and sumsq >= 0 else float("nan")
        c = self.max_grad_norm / (norm + 1e-6)
        coef = c if (c < 1.0 or c != c) else 1.0
        self.grad_norm_device.copy_(torch.tensor([sumsq, norm, coef, self.max_grad_norm], dtype=torch.float64))
        return coef

    def _tail_args(self, coef) -> dict:
        """What a flat-buffer step takes beyond the plain one: the clip coefficient (None: off) and the
        arena's EMA buffer (None: off) with its decay."""
        return dict(coef=coef, ema=self.ema[0] if self.ema else None, ema_decay=self.ema_decay)

    def _ema_torch(self, i, p):
        if self.ema is not None:
            self.ema[i].mul_(self.ema_decay).add_((1.0 - self.ema_decay) * p)

    def last_grad_norm(self) -> Optional[float]:
        """The gradient norm of the last step (before clipping), read on the host: a device
        synchronisation, so not for the hot path. None when clipping is off."""
        return None if self.grad_norm_device is None else float(self.grad_norm_device[1].item())

    @contextlib.contextmanager
    def ema_weights(self):
        """Run the body on the EMA weights: the flat master buffer and the EMA buffer are exchanged
        (one launch, which also refreshes the bf16 shadow), the derived weight operands the model
        caches are invalidated, and on exit everything is exchanged back bit for bit. Use it
        between steps only, never inside one. BatchNorm running statistics are not averaged: the
        body sees the live ones. No-op when the EMA is off."""
        if self.ema is None:
            yield
            return
        self._swap_ema()
        try:
            yield
        finally:
            self._swap_ema()

    def _swap_ema(self):
        if self.arena is not None:
            if self._flat_p.is_cuda:
                from ..ops import hip
                hip.ema_swap(self._flat_p, self.ema[0], self.arena.shadow)
                self.arena.mark_synced()
            else:
                from ..ops import cpu
                cpu.ema_swap(self._flat_p, self.ema[0])
                self.arena.sync_shadow(force=True)
        else:
            with torch.no_grad():
                for p, e in zip(self.params, self.ema):
                    t = p.detach().clone()
                    p.copy_(e)
                    e.copy_(t)
        tr = getattr(self._model, "_transposer", None)
        if tr is not None:
            tr.invalidate()  # dgrad weight operands: regenerated from the weights by the next step

    def _tail_state(self) -> dict:
        return {"ema": [e.detach().cpu() for e in self.ema]} if self.ema else {}

    def _load_tail_state(self, d: dict) -> None:
        for dst, src in zip(self.ema or [], d.get("ema", [])):
            dst.copy_(src)

    def clear_gradients(self) -> None:
        if self.arena is not None:
            self.arena.zero_grad()
        else:
            for g in self.grads:
                g.zero_()

    zero_grad = clear_gradients

    def set_learning_rate(self, lr: float) -> None:
        if float(lr) != self.learning_rate:
            self._hyper_dirty = True
        self.learning_rate = float(lr)

    def get_learning_rate(self) -> float:
        return self.learning_rate

    _HYPER_SLOTS = 8

    def _device_hyper(self, vals):
        """Device copy of step scalars (read by the kernel; graph-replay safe).

        Uploaded from a ring of pinned host slots with an asynchronous copy: a pageable copy
        would be staged synchronously and stall the host until the stream drains, so the next
        step's graph launches could not run ahead of the GPU. A slot is rewritten only after the
        event of its previous copy has completed (eight steps earlier, in practice never waits).
        """
        dev = self._flat_p.device
        if self._hyper is None:
            self._hyper = torch.zeros(4, dtype=torch.float32, device=dev)
            self._hyper_host = torch.zeros(self._HYPER_SLOTS, 4, dtype=torch.float32).pin_memory()
            self._hyper_ev = [None] * self._HYPER_SLOTS
            self._hyper_i = 0
        k = self._hyper_i
        self._hyper_i = (k + 1) % self._HYPER_SLOTS
        if self._hyper_ev[k] is not None:
            self._hyper_ev[k].synchronize()
        slot = self._hyper_host[k]
        slot.copy_(torch.tensor(list(vals) + [0.0] * (4 - len(vals)), dtype=torch.float32))
        # the copy and the event that guards the pinned slot go on the SAME stream: the current
        # stream of the arena's device (a pipeline stage thread may have another device current)
        s = torch.cuda.current_stream(dev)
        with torch.cuda.stream(s):
            self._hyper.copy_(slot, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(s)
        self._hyper_ev[k] = ev
        return self._hyper

    def _upload_hyper(self, vals):
        """Fused path: upload the step scalars only when stale (first step, re-attach, learning-rate
        change, loaded state)."""
        if self.fused() and (self._hyper_dirty or self._hyper is None):
            self._device_hyper(vals)
            self._hyper_dirty = False

    def name(self) -> str:
        return type(self).__name__

    def get_config(self) -> OptimizerConfig:
        """Type string (the lower-case name, a key of ``_KINDS``) and that class's constructor arguments."""
        kind = self.name().lower()
        return OptimizerConfig(kind, self.name(), {k: getattr(self, k) for k in _hyper_names(_KINDS[kind])})

    def clone(self) -> "Optimizer":
        return OptimizerFactory.create_from_config(self.get_config())

    def state_dict(self) -> dict:
        return {}

    def load_state_dict(self, d: dict) -> None:
        pass


def _hyper_names(cls) -> List[str]:
    """The hyper-parameters of an optimizer class: its constructor's arguments, each kept as an
    attribute of the same name."""
    return [k for k in inspect.signature(cls.__init__).parameters if k != "self"]


def _zeros_like_params(opt) -> List[torch.Tensor]:
    """One state buffer: flat over the arena, else one tensor per parameter."""
    return [opt.arena.new_zeros()] if opt.arena is not None else [torch.zeros_like(p) for p in opt.params]


def _copy_state(dst, src) -> None:
    for d, s in zip(dst or [], src or []):
        d.copy_(s)


class _VelocityState(Optimizer):
    """SGD's and LARS's state: ``velocity`` (none with momentum 0) and the device scalars ``{lr}``."""

    def __init__(self, learning_rate, momentum, max_grad_norm, ema_decay):
        super().__init__(learning_rate, max_grad_norm, ema_decay)
        self.momentum = float(momentum)
        self.velocity = None

    def _on_attach(self):
        self.velocity = _zeros_like_params(self) if self.momentum > 0 else None

    def _vel(self, i=0):
        return self.velocity[i] if self.momentum > 0 else None

    def prepare_step(self):
        self._upload_hyper([self.learning_rate])

    def state_dict(self):
        return {"velocity": [v.detach().cpu() for v in self.velocity or []], **self._tail_state()}

    def load_state_dict(self, d):
        self._load_tail_state(d)
        _copy_state(self.velocity, d.get("velocity"))


class _MomentState(Optimizer):
    """Adam's and LAMB's state: the step count ``t``, the moments ``m`` and ``v``, and the device
    scalars ``{lr, bc1, bc2, t}``."""

    def __init__(self, learning_rate, beta1, beta2, epsilon, max_grad_norm, ema_decay):
        super().__init__(learning_rate, max_grad_norm, ema_decay)
        self.beta1, self.beta2, self.epsilon = float(beta1), float(beta2), float(epsilon)
        self.t = 0
        self.m = self.v = None

    def _on_attach(self):
        self.m, self.v = _zeros_like_params(self), _zeros_like_params(self)
        self.t = 0

    def prepare_step(self):
        """Advance the host step counter and take the bias corrections; upload the device scalars only
        when stale — the device counter then equals t - 1 and ``launch_step`` advances it on the
        device (``adam_scalars`` / ``lamb_scalars``)."""
        self.t += 1
        self._bc = (1.0 - self.beta1 ** self.t, 1.0 - self.beta2 ** self.t)
        self._upload_hyper([self.learning_rate, 0.0, 0.0, float(self.t - 1)])

    def _moments_torch(self, i, g):
        """Parameter ``i`` in torch: m, v <- g; returns ``m_hat`` and ``sqrt(v_hat) + eps``."""
        m, v = self.m[i], self.v[i]
        m.mul_(self.beta1).add_((1 - self.beta1) * g)
        v.mul_(self.beta2).add_((1 - self.beta2) * g * g)
        return m / self._bc[0], torch.sqrt(v / self._bc[1]) + self.epsilon

    def state_dict(self):
        return {"t": self.t, "m": [x.detach().cpu() for x in self.m or []], "v": [x.detach().cpu() for x in self.v or []],
                **self._tail_state()}

    def load_state_dict(self, d):
        self._load_tail_state(d)
        self.t = int(d.get("t", 0))
        self._hyper_dirty = True
        _copy_state(self.m, d.get("m"))
        _copy_state(self.v, d.get("v"))


class SGD(_VelocityState):
    def __init__(self, learning_rate: float = 0.01, momentum: float = 0.0, max_grad_norm: float = 0.0,
                 ema_decay: float = 0.0):
        super().__init__(learning_rate, momentum, max_grad_norm, ema_decay)

    def launch_step(self):
        from ..ops import hip
        args = (self._flat_p, self._flat_g, self._vel(), self.arena.shadow, self.learning_rate, self.momentum,
                self._hyper)
        if self._tail():
            hip.sgd_step_tail(*args, **self._tail_args(self._launch_norm()))
        else:
            hip.sgd_step(*args)
        self.arena.mark_synced()

    def _step_cpu_arena(self, cpu):
        args = (self._flat_p, self._flat_g, self._vel(), self.learning_rate, self.momentum)
        if self._tail():
            cpu.sgd_step_tail(*args, **self._tail_args(self._host_coef()))
        else:
            cpu.sgd_step(*args)

    def _step_param(self, i, p, g):
        v = self._vel(i)
        if v is not None:
            v.mul_(self.momentum).sub_(self.learning_rate * g)
            p.add_(v)
        else:
            p.sub_(self.learning_rate * g)


class Adam(_MomentState):
    def __init__(self, learning_rate: float = 0.001, beta1: float = 0.9, beta2: float = 0.999,
                 epsilon: float = 1e-8, weight_decay: float = 0.0, decouple_weight_decay: bool = False,
                 no_decay_norm_bias: bool = False, max_grad_norm: float = 0.0, ema_decay: float = 0.0):
        """``no_decay_norm_bias``: biases, norm affines and layer scales take the step without
        weight decay. On the fused arena path a static device table of one byte per 64-element
        block selects them inside the one launch; off (the default), the launch is unchanged.
        ``max_grad_norm`` / ``ema_decay``: global-norm clipping and the weight EMA (module docstring);
        with either on, the step is the norm reduction plus one instance of the step kernel that
        reads the coefficient and maintains the EMA."""
        super().__init__(learning_rate, beta1, beta2, epsilon, max_grad_norm, ema_decay)
        self.no_decay_norm_bias = bool(no_decay_norm_bias)
        self.weight_decay = float(weight_decay)
        self.decouple_weight_decay = bool(decouple_weight_decay)

    def _on_attach(self):
        super()._on_attach()
        self._need_no_decay_flags()
        on = self.no_decay_norm_bias and self.arena is not None
        self._nodecay_blocks = self.arena.no_decay_blocks() if on else None

    def _scalars(self):
        return (self.learning_rate, self.beta1, self.beta2, self.epsilon, *self._bc, self.weight_decay,
                self.decouple_weight_decay)

    def launch_step(self):
        """The scalar update (t, bias corrections) and ONE kernel over the flat buffer."""
        from ..ops import hip
        from ..ops._ext import kernels, stream_ptr
        kernels().adam_scalars(self._hyper.data_ptr(), float(self.beta1), float(self.beta2),
                               stream_ptr(self._flat_p.device))
        args = (self._flat_p, self._flat_g, self.m[0], self.v[0], self.arena.shadow, *self._scalars(), self._hyper)
        if self._tail():
            hip.adam_step_tail(*args, nodecay=self._nodecay_blocks, **self._tail_args(self._launch_norm()))
        else:
            hip.adam_step(*args, nodecay=self._nodecay_blocks)
        self.arena.mark_synced()

    def _step_cpu_arena(self, cpu):
        args = (self._flat_p, self._flat_g, self.m[0], self.v[0], *self._scalars())
        if self._tail():
            cpu.adam_step_tail(*args, nodecay=self._nodecay_blocks, **self._tail_args(self._host_coef()))
        elif self._nodecay_blocks is not None:
            cpu.adam_step_nodecay(*args, self._nodecay_blocks)
        else:
            cpu.adam_step(*args)

    def _step_param(self, i, p, g):
        m_hat, denom = self._moments_torch(i, g)
        upd = self.learning_rate * m_hat / denom
        wd = 0.0 if (self.no_decay_norm_bias and self.no_decay[i]) else self.weight_decay
        if wd > 0:
            if self.decouple_weight_decay:
                p.sub_(wd * self.learning_rate * p)
            else:
                upd = upd + wd * self.learning_rate * p
        p.sub_(upd)

    def name(self):
        return "AdamW" if self.decouple_weight_decay else "Adam"


class AdamW(Adam):
    def __init__(self, learning_rate=0.001, beta1=0.9, beta2=0.999, epsilon=1e-8, weight_decay=0.01,
                 no_decay_norm_bias=False, max_grad_norm=0.0, ema_decay=0.0):
        super().__init__(learning_rate, beta1, beta2, epsilon, weight_decay, True, no_decay_norm_bias, max_grad_norm,
                         ema_decay)


class _Layerwise(Optimizer):
    """What LAMB and LARS share: a trust ratio per parameter from the L2 norms of its weights and of
    its update, taken on the weights before the step. On an arena the norms are ONE segmented
    fixed-order reduction over the flat buffer (``ParamArena.segment_tables``; ``layerwise.hip`` on the
    GPU, the native loops on the CPU) and the step is two launches; the trust table stays on the
    device, so a captured step needs no host read. With ``no_decay_norm_bias`` a parameter flagged
    ``no_decay`` (biases, norm affines, layer scales) takes ``wd = 0`` and trust 1. A zero norm gives
    trust 1; a non-finite norm propagates into that parameter's step (no step is skipped)."""

    layerwise = True  # TrainStep prewarms the "layerwise" ticket slot before a capture

    def _init_layerwise(self, weight_decay, no_decay_norm_bias):
        self.weight_decay = float(weight_decay)
        self.no_decay_norm_bias = bool(no_decay_norm_bias)
        self._tables = self._trust = self._part = None

    def _on_attach(self):
        super()._on_attach()  # (the moment or velocity state)
        self._tables = self._trust = self._part = None
        self._need_no_decay_flags()
        if self.arena is not None:
            self._tables = self.arena.segment_tables(self.no_decay_norm_bias)
            if self._flat_p.is_cuda:
                from ..ops import hip
                self._trust, self._part = hip.layerwise_workspace(self._tables, self._flat_p.device)
            else:
                self._trust = torch.ones(max(3 * self._tables.nsegs, 1), dtype=torch.float64)
        else:
            self._trust = [1.0] * len(self.params)

    def _excluded(self, i) -> bool:
        return self.no_decay_norm_bias and self.no_decay[i]

    def last_trust_ratios(self) -> List[float]:
        """The trust ratio of every parameter in the last step (1.0 before the first), read on the
        host: a device synchronisation on the GPU, so not for the hot path."""
        if self._trust is None:
            return []
        if isinstance(self._trust, list):
            return list(self._trust)
        return [float(x) for x in self._trust[:self._tables.nsegs].double().cpu().tolist()]

    def last_norm_sums(self) -> List[tuple]:
        """``(sum p^2, sum u^2)`` per parameter as the last arena step's reduction left them (u: LAMB's
        update ``r``, LARS's gradient before the clip coefficient): for inspection, a host read."""
        if self._trust is None or isinstance(self._trust, list):
            return []
        ns = self._tables.nsegs
        return [tuple(x) for x in self._trust[ns:3 * ns].double().cpu().reshape(ns, 2).tolist()]

    @staticmethod
    def _norm(t) -> float:
        return math.sqrt(float((t.detach().double() ** 2).sum()))





class LAMB(_Layerwise, _MomentState):
    """LAMB (You et al. 2019): Adam's moments, the update ``r = (m / bc1) / (sqrt(v / bc2) + eps) +
    wd p`` scaled per parameter by ``trust = ||p|| / ||r||``: ``p -= lr trust r``. State as Adam's
    (``t``, ``m``, ``v``; the device scalars advance by ``lamb_scalars``: the bias corrections in double)."""

    def __init__(self, learning_rate: float = 1e-3, beta1: float = 0.9, beta2: float = 0.999, epsilon: float = 1e-6,
                 weight_decay: float = 0.01, no_decay_norm_bias: bool = False, max_grad_norm: float = 0.0,
                 ema_decay: float = 0.0):
        super().__init__(learning_rate, beta1, beta2, epsilon, max_grad_norm, ema_decay)
        self._init_layerwise(weight_decay, no_decay_norm_bias)

    def _scalars(self):
        return (self.learning_rate, self.beta1, self.beta2, self.epsilon, *self._bc, self.weight_decay)

    def launch_step(self):
        from ..ops import hip
        from ..ops._ext import kernels, stream_ptr
        kernels().lamb_scalars(self._hyper.data_ptr(), float(self.beta1), float(self.beta2),
                               stream_ptr(self._flat_p.device))
        hip.lamb_step(self._flat_p, self._flat_g, self.m[0], self.v[0], self.arena.shadow, *self._scalars(),
                      self._tables, self._trust, self._part, hyper=self._hyper,
                      **self._tail_args(self._launch_norm()))
        self.arena.mark_synced()

    def _step_cpu_arena(self, cpu):
        cpu.lamb_step(self._flat_p, self._flat_g, self.m[0], self.v[0], *self._scalars(), self._tables, self._trust,
                      **self._tail_args(self._host_coef()))

    def _step_param(self, i, p, g):
        m_hat, denom = self._moments_torch(i, g)
        r = m_hat / denom
        trust = 1.0
        if not self._excluded(i):
            r = r + self.weight_decay * p
            pn, rn = self._norm(p), self._norm(r)
            trust = 1.0 if (pn == 0.0 or rn == 0.0) else pn / rn
        self._trust[i] = trust
        p.sub_(self.learning_rate * trust * r)


class LARS(_Layerwise, _VelocityState):
    """LARS (You et al. 2017): momentum SGD with L2 weight decay, the step of every parameter scaled
    by ``trust = tc ||p|| / (||g|| + wd ||p|| + eps)``: ``v = mom v - lr trust (g + wd p)``, ``p += v``
    (the velocity convention of :class:`SGD`; momentum 0: no velocity buffer). State as SGD's."""

    def __init__(self, learning_rate: float = 0.1, momentum: float = 0.9, weight_decay: float = 5e-4,
                 trust_coefficient: float = 1e-3, epsilon: float = 1e-8, no_decay_norm_bias: bool = False,
                 max_grad_norm: float = 0.0, ema_decay: float = 0.0):
        super().__init__(learning_rate, momentum, max_grad_norm, ema_decay)
        self._init_layerwise(weight_decay, no_decay_norm_bias)
        self.trust_coefficient, self.epsilon = float(trust_coefficient), float(epsilon)

    def _scalars(self):
        return (self.learning_rate, self.momentum, self.weight_decay, self.trust_coefficient, self.epsilon)

    def launch_step(self):
        from ..ops import hip
        hip.lars_step(self._flat_p, self._flat_g, self._vel(), self.arena.shadow, *self._scalars(), self._tables,
                      self._trust, self._part, hyper=self._hyper, **self._tail_args(self._launch_norm()))
        self.arena.mark_synced()

    def _step_cpu_arena(self, cpu):
        cpu.lars_step(self._flat_p, self._flat_g, self._vel(), *self._scalars(), self._tables, self._trust,
                      **self._tail_args(self._host_coef()))

    def _step_param(self, i, p, g):
        trust, wd = 1.0, 0.0
        if not self._excluded(i):
            wd = self.weight_decay
            pn, gn = self._norm(p), self._norm(g)
            if not (pn == 0.0 or gn == 0.0):
                trust = self.trust_coefficient * pn / (gn + wd * pn + self.epsilon)
        self._trust[i] = trust
        u = g + wd * p
        v = self._vel(i)
        if v is not None:
            v.mul_(self.momentum).sub_(self.learning_rate * trust * u)
            p.add_(v)
        else:
            p.sub_(self.learning_rate * trust * u)


# config type string -> the class whose constructor arguments are the config's parameters
_KINDS = {"sgd": SGD, "adam": Adam, "adamw": Adam, "lamb": LAMB, "lars": LARS}


class OptimizerFactory:
    @staticmethod
    def create_from_config(config) -> Optimizer:
        """Parameters the config leaves out take the constructor's defaults, keys the constructor does
        not know are ignored. ``adamw`` is :class:`Adam` with ``decouple_weight_decay`` on by default."""
        if isinstance(config, dict) and not isinstance(config, OptimizerConfig):
            config = OptimizerConfig.from_json(config)
        t = config["type"]
        p = config["parameters"]
        if t not in _KINDS:
            raise ValueError(f"Unknown optimizer type: {t}")
        given = {k: p[k] for k in _hyper_names(_KINDS[t]) if k in p}
        if t == "adamw":
            given.setdefault("decouple_weight_decay", True)
        return _KINDS[t](**given)
