#!/usr/bin/env python3
"""ResNeXt 32x4d (bottleneck blocks with a 32-group 3x3 on the grouped-conv kernels): ResNeXt-26 on
CIFAR-10 or, with ``--tiny``, ResNeXt-50 on Tiny-ImageNet-200: crop + flip + normalize, Adam, softmax
cross-entropy. No reference counterpart (the reference has no grouped convolution)."""
from common import loaders, parse, place

from dcnn_amd.data import AugmentationBuilder
from dcnn_amd.models import create_model
from dcnn_amd.nn import Adam, LossFactory, train_classification_model
from dcnn_amd.utils import get_env

STATS = {"cifar10": ((0.49139968, 0.48215827, 0.44653124), (0.24703233, 0.24348505, 0.26158768)),
         "tiny": ((0.4802, 0.4481, 0.3975), (0.2770, 0.2691, 0.2821))}
a, cfg = parse(__doc__, lambda ap: ap.add_argument("--tiny", action="store_true",
                                                   help="ResNeXt-50 on Tiny-ImageNet-200 (64x64, 200 classes)"))
kind = "tiny" if a.tiny else "cifar10"
mean, std = STATS[kind]
tr, te = loaders(kind, a, cfg)
tr.set_augmentation(AugmentationBuilder().random_crop(0.5, 4).horizontal_flip(0.5).normalize(mean, std).build())
te.set_augmentation(AugmentationBuilder().normalize(mean, std).build())
model = place(create_model("resnext50_32x4d_tiny_imagenet" if a.tiny else "resnext26_32x4d_cifar10"), a)
opt = Adam(get_env("LR_INITIAL", 0.001), 0.9, 0.999, 1e-8, 1e-4)
train_classification_model(model, tr, te, opt, LossFactory.create("softmax_crossentropy"), cfg)
