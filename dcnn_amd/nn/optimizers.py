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

    def update(self) -> None:
        raise NotImplementedError

    step = property(lambda self: self.update)

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

    def state_dict(self) -> dict:
        return {}

    def load_state_dict(self, d: dict) -> None:
        pass


class SGD(Optimizer):
    def __init__(self, learning_rate: float = 0.01, momentum: float = 0.0, max_grad_norm: float = 0.0,
                 ema_decay: float = 0.0):
        super().__init__(learning_rate, max_grad_norm, ema_decay)
        self.momentum = float(momentum)
        self.velocity = None

    def _on_attach(self):
        if self.momentum > 0:
            if self.arena is not None:
                self.velocity = [self.arena.new_zeros()]
            else:
                self.velocity = [torch.zeros_like(p) for p in self.params]

    def prepare_step(self):
        if self.arena is not None and self._flat_p.is_cuda and (self._hyper_dirty or self._hyper is None):
            self._device_hyper([self.learning_rate])
            self._hyper_dirty = False

    def launch_step(self):
        from ..ops import hip
        vel = self.velocity[0] if self.momentum > 0 else None
        if self._tail():
            hip.sgd_step_tail(self._flat_p, self._flat_g, vel, self.arena.shadow, self.learning_rate, self.momentum,
                              self._hyper, self._launch_norm(), self.ema[0] if self.ema else None, self.ema_decay)
        else:
            hip.sgd_step(self._flat_p, self._flat_g, vel, self.arena.shadow, self.learning_rate, self.momentum,
                         self._hyper)
        self.arena.mark_synced()

    def fused(self) -> bool:
        return self.arena is not None and self._flat_p.is_cuda

    def update(self):
        if self.arena is not None:
            p, g = self._flat_p, self._flat_g
            if p.is_cuda:
                self.prepare_step()
                self.launch_step()
                return
            from ..ops import cpu
            vel = self.velocity[0] if self.momentum > 0 else None
            if self._tail():
                cpu.sgd_step_tail(p, g, vel, self.learning_rate, self.momentum, self._host_coef(),
                                  self.ema[0] if self.ema else None, self.ema_decay)
            else:
                cpu.sgd_step(p, g, vel, self.learning_rate, self.momentum)
            self.arena.sync_shadow()
            return
        coef = self._host_coef()  # over all parameters, before any of them is stepped
        for i, (p, g) in enumerate(zip(self.params, self.grads)):
            self._sgd_torch(p, g if coef is None else g * coef, self.velocity[i] if self.momentum > 0 else None)
            with torch.no_grad():
                self._ema_torch(i, p)

    def _sgd_torch(self, p, g, v):
        with torch.no_grad():
            if v is not None:
                v.mul_(self.momentum).sub_(self.learning_rate * g)
                p.add_(v)
            else:
                p.sub_(self.learning_rate * g)

    def name(self):
        return "SGD"

    def get_config(self):
        return OptimizerConfig("sgd", "SGD", {"learning_rate": self.learning_rate, "momentum": self.momentum,
                                              "max_grad_norm": self.max_grad_norm, "ema_decay": self.ema_decay})

    def clone(self):
        return SGD(self.learning_rate, self.momentum, self.max_grad_norm, self.ema_decay)

    def state_dict(self):
        return {"velocity": [v.detach().cpu() for v in self.velocity] if self.velocity else [], **self._tail_state()}

    def load_state_dict(self, d):
        self._load_tail_state(d)
        if d.get("velocity") and self.velocity:
            for v, s in zip(self.velocity, d["velocity"]):
                v.copy_(s)


class Adam(Optimizer):
    def __init__(self, learning_rate: float = 0.001, beta1: float = 0.9, beta2: float = 0.999,
                 epsilon: float = 1e-8, weight_decay: float = 0.0, decouple_weight_decay: bool = False,
                 no_decay_norm_bias: bool = False, max_grad_norm: float = 0.0, ema_decay: float = 0.0):
        """``no_decay_norm_bias``: biases, norm affines and layer scales take the step without
        weight decay. On the fused arena path a static device table of one byte per 64-element
        block selects them inside the one launch; off (the default), the launch is unchanged.
        ``max_grad_norm`` / ``ema_decay``: global-norm clipping and the weight EMA (module docstring);
        with either on, the step is the norm reduction plus one instance of the step kernel that
        reads the coefficient and maintains the EMA."""
        super().__init__(learning_rate, max_grad_norm, ema_decay)
        self.no_decay_norm_bias = bool(no_decay_norm_bias)
        self.beta1, self.beta2, self.epsilon = float(beta1), float(beta2), float(epsilon)
        self.weight_decay = float(weight_decay)
        self.decouple_weight_decay = bool(decouple_weight_decay)
        self.t = 0
        self.m = self.v = None

    def _on_attach(self):
        if self.arena is not None:
            self.m = [self.arena.new_zeros()]
            self.v = [self.arena.new_zeros()]
        else:
            self.m = [torch.zeros_like(p) for p in self.params]
            self.v = [torch.zeros_like(p) for p in self.params]
        self.t = 0
        self._nodecay_blocks = None
        if self.no_decay_norm_bias:
            if self.no_decay is None:
                raise ValueError("no_decay_norm_bias needs to know which parameters are biases, norm affines or "
                                 "layer scales: attach a model or an arena, or pass no_decay=[...]")
            if self.arena is not None:
                self._nodecay_blocks = self.arena.no_decay_blocks()

    def fused(self) -> bool:
        return self.arena is not None and self._flat_p.is_cuda

    def prepare_step(self):
        """Host side of a step (graph-replay safe): advance the host step counter; upload the
        device scalars only when stale (first step, learning-rate change, loaded state) — the
        device counter then equals t - 1 and ``launch_step`` advances it on the device."""
        self.t += 1
        self._bc = (1.0 - self.beta1 ** self.t, 1.0 - self.beta2 ** self.t)
        if self.fused() and (self._hyper_dirty or self._hyper is None):
            self._device_hyper([self.learning_rate, 0.0, 0.0, float(self.t - 1)])
            self._hyper_dirty = False

    def launch_step(self):
        """Device side: the scalar update (t, bias corrections) and ONE kernel over the flat
        buffer, both reading their scalars from device memory."""
        from ..ops import hip
        from ..ops._ext import kernels, stream_ptr
        kernels().adam_scalars(self._hyper.data_ptr(), float(self.beta1), float(self.beta2),
                               stream_ptr(self._flat_p.device))
        bc1, bc2 = self._bc
        args = (self._flat_p, self._flat_g, self.m[0], self.v[0], self.arena.shadow, self.learning_rate, self.beta1,
                self.beta2, self.epsilon, bc1, bc2, self.weight_decay, self.decouple_weight_decay, self._hyper)
        if self._tail():
            hip.adam_step_tail(*args, nodecay=self._nodecay_blocks, coef=self._launch_norm(),
                               ema=self.ema[0] if self.ema else None, ema_decay=self.ema_decay)
        else:
            hip.adam_step(*args, nodecay=self._nodecay_blocks)
        self.arena.mark_synced()

    def update(self):
        if self.fused():
            self.prepare_step()
            self.launch_step()
            return
        self.t += 1
        bc1 = 1.0 - self.beta1 ** self.t
        bc2 = 1.0 - self.beta2 ** self.t
        if self.arena is not None and not self._flat_p.is_cuda:
            from ..ops import cpu   # native flat-buffer step (CPU arena, float32 or float64)
            args = (self._flat_p, self._flat_g, self.m[0], self.v[0], self.learning_rate, self.beta1, self.beta2,
                    self.epsilon, bc1, bc2, self.weight_decay, self.decouple_weight_decay)
            if self._tail():
                cpu.adam_step_tail(*args, self._nodecay_blocks, self._host_coef(), self.ema[0] if self.ema else None,
                                   self.ema_decay)
            elif self._nodecay_blocks is not None:
                cpu.adam_step_nodecay(*args, self._nodecay_blocks)
            else:
                cpu.adam_step(*args)
            self.arena.sync_shadow()
            return
        pairs = [(self._flat_p, self._flat_g)] if self.arena is not None else list(zip(self.params, self.grads))
        coef = self._host_coef()  # over all parameters, before any of them is stepped
        with torch.no_grad():
            for i, (p, g) in enumerate(pairs):
                m, v = self.m[i], self.v[i]
                if coef is not None:
                    g = g * coef
                m.mul_(self.beta1).add_((1 - self.beta1) * g)
                v.mul_(self.beta2).add_((1 - self.beta2) * g * g)
                upd = self.learning_rate * (m / bc1) / (torch.sqrt(v / bc2) + self.epsilon)
                wd = 0.0 if (self.no_decay_norm_bias and self.arena is None and self.no_decay[i]) else self.weight_decay
                if wd > 0:
                    if self.decouple_weight_decay:
                        p.sub_(wd * self.learning_rate * p)
                    else:
                        upd = upd + wd * self.learning_rate * p
                p.sub_(upd)
                self._ema_torch(i, p)
        if self.arena is not None:
            self.arena.sync_shadow()

    def name(self):
        return "AdamW" if self.decouple_weight_decay else "Adam"

    def get_config(self):
        t = "adamw" if self.decouple_weight_decay else "adam"
        return OptimizerConfig(t, self.name(), dict(learning_rate=self.learning_rate, beta1=self.beta1,
                                                    beta2=self.beta2, epsilon=self.epsilon,
                                                    weight_decay=self.weight_decay,
                                                    decouple_weight_decay=self.decouple_weight_decay,
                                                    no_decay_norm_bias=self.no_decay_norm_bias,
                                                    max_grad_norm=self.max_grad_norm, ema_decay=self.ema_decay))

    def clone(self):
        return Adam(self.learning_rate, self.beta1, self.beta2, self.epsilon, self.weight_decay,
                    self.decouple_weight_decay, self.no_decay_norm_bias, self.max_grad_norm, self.ema_decay)

    def state_dict(self):
        return {"t": self.t, "m": [x.detach().cpu() for x in self.m or []], "v": [x.detach().cpu() for x in self.v or []],
                **self._tail_state()}

    def load_state_dict(self, d):
        self._load_tail_state(d)
        self.t = int(d.get("t", 0))
        self._hyper_dirty = True
        for dst, src in zip(self.m or [], d.get("m", [])):
            dst.copy_(src)
        for dst, src in zip(self.v or [], d.get("v", [])):
            dst.copy_(src)


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

    def _attach_layerwise(self):
        self._tables = self._trust = self._part = None
        if self.no_decay_norm_bias and self.no_decay is None:
            raise ValueError("no_decay_norm_bias needs to know which parameters are biases, norm affines or "
                             "layer scales: attach a model or an arena, or pass no_decay=[...]")
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

    def fused(self) -> bool:
        return self.arena is not None and self._flat_p.is_cuda

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


class LAMB(_Layerwise):
    """LAMB (You et al. 2019): Adam's moments, the update ``r = (m / bc1) / (sqrt(v / bc2) + eps) +
    wd p`` scaled per parameter by ``trust = ||p|| / ||r||``: ``p -= lr trust r``. State as Adam's
    (``t``, ``m``, ``v``)."""

    def __init__(self, learning_rate: float = 1e-3, beta1: float = 0.9, beta2: float = 0.999, epsilon: float = 1e-6,
                 weight_decay: float = 0.01, no_decay_norm_bias: bool = False, max_grad_norm: float = 0.0,
                 ema_decay: float = 0.0):
        super().__init__(learning_rate, max_grad_norm, ema_decay)
        self._init_layerwise(weight_decay, no_decay_norm_bias)
        self.beta1, self.beta2, self.epsilon = float(beta1), float(beta2), float(epsilon)
        self.t = 0
        self.m = self.v = None

    def _on_attach(self):
        if self.arena is not None:
            self.m = [self.arena.new_zeros()]
            self.v = [self.arena.new_zeros()]
        else:
            self.m = [torch.zeros_like(p) for p in self.params]
            self.v = [torch.zeros_like(p) for p in self.params]
        self.t = 0
        self._attach_layerwise()

    def prepare_step(self):
        """As ``Adam.prepare_step``: the host counter advances, the device scalars are uploaded only
        when stale and advance on the device (``lamb_scalars``: the bias corrections in double)."""
        self.t += 1
        self._bc = (1.0 - self.beta1 ** self.t, 1.0 - self.beta2 ** self.t)
        if self.fused() and (self._hyper_dirty or self._hyper is None):
            self._device_hyper([self.learning_rate, 0.0, 0.0, float(self.t - 1)])
            self._hyper_dirty = False

    def launch_step(self):
        from ..ops import hip
        from ..ops._ext import kernels, stream_ptr
        kernels().lamb_scalars(self._hyper.data_ptr(), float(self.beta1), float(self.beta2),
                               stream_ptr(self._flat_p.device))
        bc1, bc2 = self._bc
        hip.lamb_step(self._flat_p, self._flat_g, self.m[0], self.v[0], self.arena.shadow, self.learning_rate,
                      self.beta1, self.beta2, self.epsilon, bc1, bc2, self.weight_decay, self._tables, self._trust,
                      self._part, hyper=self._hyper, coef=self._launch_norm(), ema=self.ema[0] if self.ema else None,
                      ema_decay=self.ema_decay)
        self.arena.mark_synced()

    def update(self):
        if self.fused():
            self.prepare_step()
            self.launch_step()
            return
        self.t += 1
        bc1 = 1.0 - self.beta1 ** self.t
        bc2 = 1.0 - self.beta2 ** self.t
        if self.arena is not None:
            from ..ops import cpu   # native flat-buffer step (CPU arena, float32 or float64)
            cpu.lamb_step(self._flat_p, self._flat_g, self.m[0], self.v[0], self.learning_rate, self.beta1, self.beta2,
                          self.epsilon, bc1, bc2, self.weight_decay, self._tables, self._trust, self._host_coef(),
                          self.ema[0] if self.ema else None, self.ema_decay)
            self.arena.sync_shadow()
            return
        coef = self._host_coef()  # over all parameters, before any of them is stepped
        with torch.no_grad():
            for i, (p, g) in enumerate(zip(self.params, self.grads)):
                m, v = self.m[i], self.v[i]
                if coef is not None:
                    g = g * coef
                m.mul_(self.beta1).add_((1 - self.beta1) * g)
                v.mul_(self.beta2).add_((1 - self.beta2) * g * g)
                r = (m / bc1) / (torch.sqrt(v / bc2) + self.epsilon)
                trust = 1.0
                if not self._excluded(i):
                    r = r + self.weight_decay * p
                    pn, rn = self._norm(p), self._norm(r)
                    trust = 1.0 if (pn == 0.0 or rn == 0.0) else pn / rn
                self._trust[i] = trust
                p.sub_(self.learning_rate * trust * r)
                self._ema_torch(i, p)

    def name(self):
        return "LAMB"

    def get_config(self):
        return OptimizerConfig("lamb", "LAMB", dict(learning_rate=self.learning_rate, beta1=self.beta1,
                                                    beta2=self.beta2, epsilon=self.epsilon,
                                                    weight_decay=self.weight_decay,
                                                    no_decay_norm_bias=self.no_decay_norm_bias,
                                                    max_grad_norm=self.max_grad_norm, ema_decay=self.ema_decay))

    def clone(self):
        return LAMB(self.learning_rate, self.beta1, self.beta2, self.epsilon, self.weight_decay,
                    self.no_decay_norm_bias, self.max_grad_norm, self.ema_decay)

    state_dict = Adam.state_dict
    load_state_dict = Adam.load_state_dict


class LARS(_Layerwise):
    """LARS (You et al. 2017): momentum SGD with L2 weight decay, the step of every parameter scaled
    by ``trust = tc ||p|| / (||g|| + wd ||p|| + eps)``: ``v = mom v - lr trust (g + wd p)``, ``p += v``
    (the velocity convention of :class:`SGD`; momentum 0: no velocity buffer). State as SGD's."""

    def __init__(self, learning_rate: float = 0.1, momentum: float = 0.9, weight_decay: float = 5e-4,
                 trust_coefficient: float = 1e-3, epsilon: float = 1e-8, no_decay_norm_bias: bool = False,
                 max_grad_norm: float = 0.0, ema_decay: float = 0.0):
        super().__init__(learning_rate, max_grad_norm, ema_decay)
        self._init_layerwise(weight_decay, no_decay_norm_bias)
        self.momentum = float(momentum)
        self.trust_coefficient, self.epsilon = float(trust_coefficient), float(epsilon)
        self.velocity = None

    def _on_attach(self):
        self.velocity = None
        if self.momentum > 0:
            if self.arena is not None:
                self.velocity = [self.arena.new_zeros()]
            else:
                self.velocity = [torch.zeros_like(p) for p in self.params]
        self._attach_layerwise()

    def prepare_step(self):
        if self.fused() and (self._hyper_dirty or self._hyper is None):
            self._device_hyper([self.learning_rate])
            self._hyper_dirty = False

    def launch_step(self):
        from ..ops import hip
        hip.lars_step(self._flat_p, self._flat_g, self.velocity[0] if self.momentum > 0 else None, self.arena.shadow,
                      self.learning_rate, self.momentum, self.weight_decay, self.trust_coefficient, self.epsilon,
                      self._tables, self._trust, self._part, hyper=self._hyper, coef=self._launch_norm(),
                      ema=self.ema[0] if self.ema else None, ema_decay=self.ema_decay)
        self.arena.mark_synced()

    def update(self):
        if self.fused():
            self.prepare_step()
            self.launch_step()
            return
        if self.arena is not None:
            from ..ops import cpu
            cpu.lars_step(self._flat_p, self._flat_g, self.velocity[0] if self.momentum > 0 else None,
                          self.learning_rate, self.momentum, self.weight_decay, self.trust_coefficient, self.epsilon,
                          self._tables, self._trust, self._host_coef(), self.ema[0] if self.ema else None,
                          self.ema_decay)
            self.arena.sync_shadow()
            return
        coef = self._host_coef()  # over all parameters, before any of them is stepped
        with torch.no_grad():
            for i, (p, g) in enumerate(zip(self.params, self.grads)):
                if coef is not None:
                    g = g * coef
                trust, wd = 1.0, 0.0
                if not self._excluded(i):
                    wd = self.weight_decay
                    pn, gn = self._norm(p), self._norm(g)
                    if not (pn == 0.0 or gn == 0.0):
                        trust = self.trust_coefficient * pn / (gn + wd * pn + self.epsilon)
                self._trust[i] = trust
                u = g + wd * p
                if self.momentum > 0:
                    self.velocity[i].mul_(self.momentum).sub_(self.learning_rate * trust * u)
                    p.add_(self.velocity[i])
                else:
                    p.sub_(self.learning_rate * trust * u)
                self._ema_torch(i, p)

    def name(self):
        return "LARS"

    def get_config(self):
        return OptimizerConfig("lars", "LARS", dict(learning_rate=self.learning_rate, momentum=self.momentum,
                                                    weight_decay=self.weight_decay,
                                                    trust_coefficient=self.trust_coefficient, epsilon=self.epsilon,
                                                    no_decay_norm_bias=self.no_decay_norm_bias,
                                                    max_grad_norm=self.max_grad_norm, ema_decay=self.ema_decay))

    def clone(self):
        return LARS(self.learning_rate, self.momentum, self.weight_decay, self.trust_coefficient, self.epsilon,
                    self.no_decay_norm_bias, self.max_grad_norm, self.ema_decay)

    state_dict = SGD.state_dict
    load_state_dict = SGD.load_state_dict


class OptimizerFactory:
    @staticmethod
    def create_from_config(config) -> Optimizer:
        if isinstance(config, dict) and not isinstance(config, OptimizerConfig):
            config = OptimizerConfig.from_json(config)
        t = config["type"]
        p = config["parameters"]
        if t == "sgd":
            return SGD(p.get("learning_rate", 0.01), p.get("momentum", 0.0), p.get("max_grad_norm", 0.0),
                       p.get("ema_decay", 0.0))
        if t in ("adam", "adamw"):
            return Adam(p.get("learning_rate", 0.001), p.get("beta1", 0.9), p.get("beta2", 0.999),
                        p.get("epsilon", 1e-8), p.get("weight_decay", 0.0),
                        p.get("decouple_weight_decay", t == "adamw"), p.get("no_decay_norm_bias", False),
                        p.get("max_grad_norm", 0.0), p.get("ema_decay", 0.0))
        if t == "lamb":
            return LAMB(p.get("learning_rate", 1e-3), p.get("beta1", 0.9), p.get("beta2", 0.999),
                        p.get("epsilon", 1e-6), p.get("weight_decay", 0.01), p.get("no_decay_norm_bias", False),
                        p.get("max_grad_norm", 0.0), p.get("ema_decay", 0.0))
        if t == "lars":
            return LARS(p.get("learning_rate", 0.1), p.get("momentum", 0.9), p.get("weight_decay", 5e-4),
                        p.get("trust_coefficient", 1e-3), p.get("epsilon", 1e-8), p.get("no_decay_norm_bias", False),
                        p.get("max_grad_norm", 0.0), p.get("ema_decay", 0.0))
        raise ValueError(f"Unknown optimizer type: {t}")
