#!/usr/bin/env python3
"""ConvNeXt (7x7 depthwise conv, channel LayerNorm, 1x1 convs with GELU, layer scale; Liu et al.
2022): ConvNeXt-pico on CIFAR-10 or, with ``--tiny``, ConvNeXt-T on Tiny-ImageNet-200: crop + flip +
normalize, AdamW (``--opt lamb``: LAMB, the large-batch recipe's optimizer, same weight decay), softmax
cross-entropy. ``--mixup A`` / ``--cutmix A`` / ``--label-smoothing E`` turn on the
rest of the published recipe (0.8 / 1.0 / 0.1): batches are mixed on the device and the loss becomes
``soft_crossentropy``; ``--clip-grad N`` clips the global gradient norm inside the optimizer step and
``--model-ema D`` keeps an exponential moving average of the weights there (validation then runs on the
averaged weights; BatchNorm statistics, which ConvNeXt does not have, would not be averaged). ``--steps N`` is a smoke mode: N training steps on
synthetic data and the losses printed. No reference counterpart (the reference has no LayerNorm, GELU
or depthwise convolution)."""
import torch
from common import loaders, parse, place

from dcnn_amd.data import AugmentationBuilder, BatchMixer
from dcnn_amd.models import INPUT_SHAPES, NUM_CLASSES, create_model
from dcnn_amd.nn import LAMB, AdamW, LossFactory, train_classification_model
from dcnn_amd.utils import get_env

STATS = {"cifar10": ((0.49139968, 0.48215827, 0.44653124), (0.24703233, 0.24348505, 0.26158768)),
         "tiny": ((0.4802, 0.4481, 0.3975), (0.2770, 0.2691, 0.2821))}


def _args(ap):
    ap.add_argument("--tiny", action="store_true", help="ConvNeXt-T on Tiny-ImageNet-200 (64x64, 200 classes)")
    ap.add_argument("--steps", type=int, default=0, help="smoke mode: this many steps on synthetic data")
    ap.add_argument("--drop-path", type=float, default=0.0,
                    help="stochastic depth: the rate of the last block, rising linearly from 0 (ConvNeXt-T: 0.1)")
    ap.add_argument("--opt", choices=["adamw", "lamb"], default="adamw",
                    help="lamb: layer-wise trust ratios on Adam's update (large global batches)")
    ap.add_argument("--no-decay-norm-bias", action="store_true",
                    help="keep biases, norm affines and layer scales out of the weight decay (LAMB: and out of "
                         "the trust ratio)")
    ap.add_argument("--mixup", type=float, default=None, help="Mixup alpha (ConvNeXt: 0.8); default MIXUP_ALPHA or 0")
    ap.add_argument("--cutmix", type=float, default=None, help="CutMix alpha (ConvNeXt: 1.0); default CUTMIX_ALPHA or 0")
    ap.add_argument("--label-smoothing", type=float, default=None,
                    help="label smoothing of the loss (ConvNeXt: 0.1); default LABEL_SMOOTHING or 0")
    ap.add_argument("--clip-grad", type=float, default=None,
                    help="global-norm gradient clipping at this L2 norm; default MAX_GRAD_NORM or 0 (off)")
    ap.add_argument("--model-ema", type=float, default=None,
                    help="decay of the weight EMA (ConvNeXt: 0.9999); default EMA_DECAY or 0 (off)")


a, cfg = parse(__doc__, _args)
if a.mixup is not None:
    cfg.mixup_alpha = a.mixup
if a.cutmix is not None:
    cfg.cutmix_alpha = a.cutmix
if a.label_smoothing is not None:
    cfg.label_smoothing = a.label_smoothing
if a.clip_grad is not None:
    cfg.max_grad_norm = a.clip_grad
if a.model_ema is not None:
    cfg.ema_decay = a.model_ema
soft = cfg.mixup_alpha > 0 or cfg.cutmix_alpha > 0 or cfg.label_smoothing > 0
kind = "tiny" if a.tiny else "cifar10"
name = "convnext_tiny_tiny_imagenet" if a.tiny else "convnext_pico_cifar10"
model = place(create_model(name, drop_path_rate=a.drop_path), a)
if a.opt == "lamb":
    opt = LAMB(get_env("LR_INITIAL", 0.001), 0.9, 0.999, 1e-6, 0.05, no_decay_norm_bias=a.no_decay_norm_bias,
               max_grad_norm=cfg.max_grad_norm, ema_decay=cfg.ema_decay)
else:
    opt = AdamW(get_env("LR_INITIAL", 0.001), 0.9, 0.999, 1e-8, 0.05, no_decay_norm_bias=a.no_decay_norm_bias,
                max_grad_norm=cfg.max_grad_norm, ema_decay=cfg.ema_decay)
loss_fn = LossFactory.create("soft_crossentropy", label_smoothing=cfg.label_smoothing) if soft else \
    LossFactory.create("softmax_crossentropy")
if a.steps > 0:
    opt.attach(model)
    dev = model.get_device().torch_device
    g = torch.Generator().manual_seed(0)
    n = cfg.batch_size if a.batch_size is not None else 8
    x = torch.randn(n, *INPUT_SHAPES[name], generator=g).to(dev)
    y = torch.randint(0, NUM_CLASSES[name], (n,), generator=g).to(dev)
    mixer = BatchMixer(NUM_CLASSES[name], cfg.mixup_alpha, cfg.cutmix_alpha, cfg.mix_prob, cfg.mix_switch_prob) \
        if cfg.mixup_alpha > 0 or cfg.cutmix_alpha > 0 else None
    losses = []
    for _ in range(a.steps):
        model.clear_gradients()
        xb, yb = mixer(x.clone(), y) if mixer is not None else (x, y)
        loss, grad, _ = loss_fn.loss_and_grad(model.forward(xb), yb)
        model.backward(grad)
        opt.update()
        losses.append(float(loss))
    print(f"{name}: {model.num_parameters()} parameters, batch {n}, losses " + " ".join(f"{v:.4f}" for v in losses))
    if a.opt == "lamb":
        tr = opt.last_trust_ratios()
        print(f"last trust ratios: min {min(tr):.4f} max {max(tr):.4f} over {len(tr)} parameters")
    if opt.max_grad_norm > 0:
        print(f"last gradient norm {opt.last_grad_norm():.4f} (clipped at {opt.max_grad_norm})")
    if opt.ema is not None:
        with opt.ema_weights(), torch.no_grad():
            model.set_training(False)
            ema_loss, _, _ = loss_fn.loss_and_grad(model.forward(x), y, want_grad=False)
            model.set_training(True)
        print(f"loss on the EMA weights {float(ema_loss):.4f}")
    assert all(v == v for v in losses), "non-finite loss"
else:
    mean, std = STATS[kind]
    tr, te = loaders(kind, a, cfg)
    tr.set_augmentation(AugmentationBuilder().random_crop(0.5, 4).horizontal_flip(0.5).normalize(mean, std).build())
    te.set_augmentation(AugmentationBuilder().normalize(mean, std).build())
    train_classification_model(model, tr, te, opt, loss_fn, cfg)
