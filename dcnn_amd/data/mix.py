"""Mixup / CutMix of a training batch (Zhang et al. 2018, Yun et al. 2019; timm's ``Mixup`` in
batch mode: one lam and one box per batch, sample ``i`` mixed with sample ``B - 1 - i``).

``BatchMixer`` holds the recipe and a step counter; every random decision of training batch
``step`` is ``mix_plan(seed, step, ...)`` - one host function of the native module that both front
ends call, so a rerun or a resume (``mixer.state``) reproduces every batch. The batch itself is
mixed in place by one kernel launch (csrc/kernels/mix.hip; the native CPU backend computes the same
bits) that also writes the dense target ``[B, K]``. Targets are dense for an unmixed batch too, so a
captured step keeps one static target shape. Train against them with ``soft_crossentropy`` (which
also applies label smoothing): every other cross entropy takes its loss value from "the class above
0.5" and would report a wrong loss.
"""
from __future__ import annotations

import torch


class BatchMixer:
    def __init__(self, num_classes: int, mixup_alpha: float = 0.8, cutmix_alpha: float = 1.0, prob: float = 1.0,
                 switch_prob: float = 0.5, seed: int = 0):
        if int(num_classes) < 1:
            raise ValueError(f"BatchMixer: num_classes must be >= 1, got {num_classes}")
        if mixup_alpha < 0 or cutmix_alpha < 0:
            raise ValueError(f"BatchMixer: alphas must be >= 0, got {mixup_alpha} and {cutmix_alpha}")
        if not 0.0 <= prob <= 1.0 or not 0.0 <= switch_prob <= 1.0:
            raise ValueError(f"BatchMixer: probabilities must be in [0, 1], got {prob} and {switch_prob}")
        self.num_classes = int(num_classes)
        self.mixup_alpha = float(mixup_alpha)
        self.cutmix_alpha = float(cutmix_alpha)
        self.prob = float(prob)
        self.switch_prob = float(switch_prob)
        self.seed = int(seed)
        self._hw = None
        self.state = 0  # training batches mixed so far; the next one is step state + 1

    def plan(self, step: int, height: int = None, width: int = None):
        """``(mode, lam, yl, yh, xl, xh)`` of training batch ``step`` (from 1); no side effects.
        ``height`` / ``width`` default to the image size of the last batch mixed."""
        from ..ops import cpu
        if height is None or width is None:
            if self._hw is None:
                raise ValueError("BatchMixer.plan: give the image height and width before the first batch")
            height, width = self._hw
        return cpu.mix_plan(self.seed, step, height, width, self.mixup_alpha, self.cutmix_alpha, self.prob,
                            self.switch_prob)

    def __call__(self, x: torch.Tensor, labels: torch.Tensor):
        """Mix ``x`` [B, C, H, W] in place; returns ``(x, target [B, K] float32)`` on ``x``'s device."""
        if x.dim() != 4:
            raise ValueError("BatchMixer: x is [B, C, H, W]")
        self.state += 1
        self._hw = (int(x.shape[2]), int(x.shape[3]))
        mode, lam, yl, yh, xl, xh = self.plan(self.state, x.shape[2], x.shape[3])
        labels = labels.to(device=x.device, dtype=torch.int64).reshape(-1).contiguous()
        target = torch.empty((x.shape[0], self.num_classes), dtype=torch.float32, device=x.device)
        if x.is_cuda:
            from ..ops import hip
            hip.mix_batch(x, labels, target, mode, lam, (yl, yh, xl, xh), self.num_classes)
        else:
            from ..ops import cpu
            cpu.mix_batch(x, labels, target, mode, lam, (yl, yh, xl, xh), self.num_classes)
        return x, target

    def get_config(self) -> dict:
        return {"num_classes": self.num_classes, "mixup_alpha": self.mixup_alpha, "cutmix_alpha": self.cutmix_alpha,
                "prob": self.prob, "switch_prob": self.switch_prob, "seed": self.seed}
