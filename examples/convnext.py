#!/usr/bin/env python3
"""ConvNeXt (7x7 depthwise conv, channel LayerNorm, 1x1 convs with GELU, layer scale; Liu et al.
2022): ConvNeXt-pico on CIFAR-10 or, with ``--tiny``, ConvNeXt-T on Tiny-ImageNet-200: crop + flip +
normalize, AdamW, softmax cross-entropy. ``--steps N`` is a smoke mode: N training steps on
synthetic data and the losses printed. No reference counterpart (the reference has no LayerNorm, GELU
or depthwise convolution)."""
import torch
from common import loaders, parse, place

from dcnn_amd.data import AugmentationBuilder
from dcnn_amd.models import INPUT_SHAPES, NUM_CLASSES, create_model
from dcnn_amd.nn import AdamW, LossFactory, train_classification_model
from dcnn_amd.utils import get_env

STATS = {"cifar10": ((0.49139968, 0.48215827, 0.44653124), (0.24703233, 0.24348505, 0.26158768)),
         "tiny": ((0.4802, 0.4481, 0.3975), (0.2770, 0.2691, 0.2821))}


def _args(ap):
    ap.add_argument("--tiny", action="store_true", help="ConvNeXt-T on Tiny-ImageNet-200 (64x64, 200 classes)")
    ap.add_argument("--steps", type=int, default=0, help="smoke mode: this many steps on synthetic data")
    ap.add_argument("--drop-path", type=float, default=0.0,
                    help="stochastic depth: the rate of the last block, rising linearly from 0 (ConvNeXt-T: 0.1)")
    ap.add_argument("--no-decay-norm-bias", action="store_true",
                    help="keep biases, norm affines and layer scales out of AdamW's weight decay")


a, cfg = parse(__doc__, _args)
kind = "tiny" if a.tiny else "cifar10"
name = "convnext_tiny_tiny_imagenet" if a.tiny else "convnext_pico_cifar10"
model = place(create_model(name, drop_path_rate=a.drop_path), a)
opt = AdamW(get_env("LR_INITIAL", 0.001), 0.9, 0.999, 1e-8, 0.05, no_decay_norm_bias=a.no_decay_norm_bias)
loss_fn = LossFactory.create("softmax_crossentropy")
if a.steps > 0:
    opt.attach(model)
    dev = model.get_device().torch_device
    g = torch.Generator().manual_seed(0)
    n = cfg.batch_size if a.batch_size is not None else 8
    x = torch.randn(n, *INPUT_SHAPES[name], generator=g).to(dev)
    y = torch.randint(0, NUM_CLASSES[name], (n,), generator=g).to(dev)
    losses = []
    for _ in range(a.steps):
        model.clear_gradients()
        loss, grad, _ = loss_fn.loss_and_grad(model.forward(x), y)
        model.backward(grad)
        opt.update()
        losses.append(float(loss))
    print(f"{name}: {model.num_parameters()} parameters, batch {n}, losses " + " ".join(f"{v:.4f}" for v in losses))
    assert all(v == v for v in losses), "non-finite loss"
else:
    mean, std = STATS[kind]
    tr, te = loaders(kind, a, cfg)
    tr.set_augmentation(AugmentationBuilder().random_crop(0.5, 4).horizontal_flip(0.5).normalize(mean, std).build())
    te.set_augmentation(AugmentationBuilder().normalize(mean, std).build())
    train_classification_model(model, tr, te, opt, loss_fn, cfg)
