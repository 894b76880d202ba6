"""Model zoo: the 13 builders of the reference (`include/nn/example_models.hpp:13-437`),
same layer sequence, names and hyper-parameters, so checkpoints are interchangeable; plus
MobileNetV1 (Howard et al. 2017) on the depthwise layer and ResNeXt (Xie et al. 2017) on
the grouped layer, which the reference lacks.
"""
from __future__ import annotations

from ..nn.sequential import Sequential, SequentialBuilder


def create_mnist_trainer() -> Sequential:
    return (SequentialBuilder("mnist_cnn_model").input([1, 28, 28])
            .conv2d(8, 5, 5, 1, 1, 0, 0, True, "conv1").batchnorm(1e-5, 0.1, True, "bn1")
            .activation("relu", "relu1").maxpool2d(3, 3, 3, 3, 0, 0, "pool1")
            .conv2d(16, 1, 1, 1, 1, 0, 0, True, "conv2_1x1").batchnorm(1e-5, 0.1, True, "bn2")
            .activation("relu", "relu2")
            .conv2d(48, 5, 5, 1, 1, 0, 0, True, "conv3").batchnorm(1e-5, 0.1, True, "bn3")
            .activation("relu", "relu3").maxpool2d(2, 2, 2, 2, 0, 0, "pool2")
            .flatten("flatten").dense(10, True, "output").build())


def create_cifar10_trainer_v1() -> Sequential:
    return (SequentialBuilder("cifar10_cnn_classifier_v1").input([3, 32, 32])
            .conv2d(16, 3, 3, 1, 1, 0, 0, True, "conv1").batchnorm(1e-5, 0.1, True, "bn1")
            .activation("relu", "relu1").maxpool2d(3, 3, 3, 3, 0, 0, "maxpool1")
            .conv2d(64, 3, 3, 1, 1, 0, 0, True, "conv2").activation("relu", "relu2")
            .maxpool2d(4, 4, 4, 4, 0, 0, "maxpool2").flatten("flatten").dense(10, True, "fc1").build())


def _vgg_body(b: SequentialBuilder) -> SequentialBuilder:
    return (b.conv2d(64, 3, 3, 1, 1, 1, 1, False, "conv0").batchnorm(1e-5, 0.1, True, "bn0").activation("relu", "relu0")
            .conv2d(64, 3, 3, 1, 1, 1, 1, False, "conv1").batchnorm(1e-5, 0.1, True, "bn1").activation("relu", "relu1")
            .maxpool2d(2, 2, 2, 2, 0, 0, "pool0")
            .conv2d(128, 3, 3, 1, 1, 1, 1, False, "conv2").batchnorm(1e-5, 0.1, True, "bn2").activation("relu", "relu2")
            .conv2d(128, 3, 3, 1, 1, 1, 1, False, "conv3").batchnorm(1e-5, 0.1, True, "bn3").activation("relu", "relu3")
            .maxpool2d(2, 2, 2, 2, 0, 0, "pool1")
            .conv2d(256, 3, 3, 1, 1, 1, 1, False, "conv4").batchnorm(1e-5, 0.1, True, "bn5").activation("relu", "relu5")
            .conv2d(256, 3, 3, 1, 1, 1, 1, False, "conv5").activation("relu", "relu6")
            .conv2d(256, 3, 3, 1, 1, 1, 1, False, "conv6").batchnorm(1e-5, 0.1, True, "bn6").activation("relu", "relu6")
            .maxpool2d(2, 2, 2, 2, 0, 0, "pool2")
            .conv2d(512, 3, 3, 1, 1, 1, 1, False, "conv7").batchnorm(1e-5, 0.1, True, "bn8").activation("relu", "relu7")
            .conv2d(512, 3, 3, 1, 1, 1, 1, False, "conv8").batchnorm(1e-5, 0.1, True, "bn9").activation("relu", "relu8")
            .conv2d(512, 3, 3, 1, 1, 1, 1, False, "conv9").batchnorm(1e-5, 0.1, True, "bn10").activation("relu", "relu9")
            .maxpool2d(2, 2, 2, 2, 0, 0, "pool3").flatten("flatten"))


def create_cifar10_trainer_v2() -> Sequential:
    b = _vgg_body(SequentialBuilder("cifar10_cnn_classifier").input([3, 32, 32]))
    return b.dense(512, True, "fc0").activation("relu", "relu10").dense(10, True, "fc1").build()


def create_resnet9_cifar10() -> Sequential:
    return (SequentialBuilder("ResNet-9-CIFAR10").input([3, 32, 32])
            .conv2d(64, 3, 3, 1, 1, 1, 1, True, "conv1").batchnorm(1e-5, 0.1, True, "bn1").activation("relu", "relu1")
            .conv2d(128, 3, 3, 1, 1, 1, 1, True, "conv2").batchnorm(1e-5, 0.1, True, "bn2").activation("relu", "relu2")
            .maxpool2d(2, 2, 2, 2, 0, 0, "pool1")
            .basic_residual_block(128, 128, 1, "res_block1").basic_residual_block(128, 128, 1, "res_block2")
            .conv2d(256, 3, 3, 1, 1, 1, 1, True, "conv3").batchnorm(1e-5, 0.1, True, "bn3").activation("relu", "relu3")
            .maxpool2d(2, 2, 2, 2, 0, 0, "pool2")
            .basic_residual_block(256, 256, 1, "res_block3").basic_residual_block(256, 256, 1, "res_block4")
            .conv2d(512, 3, 3, 1, 1, 1, 1, True, "conv4").batchnorm(1e-5, 0.1, True, "bn4").activation("relu", "relu4")
            .maxpool2d(2, 2, 2, 2, 0, 0, "pool3")
            .basic_residual_block(512, 512, 1, "res_block5")
            .avgpool2d(4, 4, 1, 1, 0, 0, "avgpool").flatten("flatten").dense(10, True, "output").build())


def create_resnet18_cifar10() -> Sequential:
    b = (SequentialBuilder("ResNet-18-CIFAR10").input([3, 32, 32])
         .conv2d(64, 3, 3, 1, 1, 1, 1, True, "conv1").batchnorm(1e-5, 0.1, True, "bn1").activation("relu", "relu1")
         .basic_residual_block(64, 64, 1, "layer1_block1").basic_residual_block(64, 64, 1, "layer1_block2")
         .basic_residual_block(64, 128, 2, "layer2_block1").basic_residual_block(128, 128, 1, "layer2_block2")
         .basic_residual_block(128, 128, 1, "layer2_block3")
         .basic_residual_block(128, 256, 2, "layer3_block1").basic_residual_block(256, 256, 1, "layer3_block2")
         .basic_residual_block(256, 256, 1, "layer3_block3")
         .basic_residual_block(256, 512, 2, "layer4_block1").basic_residual_block(512, 512, 1, "layer4_block2"))
    return b.avgpool2d(4, 4, 4, 4, 0, 0, "avgpool").flatten("flatten").dense(10, True, "output").build()


def create_resnet20_cifar10() -> Sequential:
    b = (SequentialBuilder("ResNet-20-CIFAR10").input([3, 32, 32])
         .conv2d(64, 3, 3, 1, 1, 1, 1, True, "conv1").batchnorm(1e-5, 0.1, True, "bn1").activation("relu", "relu1"))
    for i in range(1, 4):
        b.basic_residual_block(64, 64, 1, f"layer1_block{i}")
    b.basic_residual_block(64, 128, 2, "layer2_block1")
    for i in range(2, 4):
        b.basic_residual_block(128, 128, 1, f"layer2_block{i}")
    b.basic_residual_block(128, 256, 2, "layer3_block1")
    for i in range(2, 4):
        b.basic_residual_block(256, 256, 1, f"layer3_block{i}")
    return b.avgpool2d(8, 8, 1, 1, 0, 0, "avgpool").flatten("flatten").dense(10, True, "output").build()


def _resnet50_body(b: SequentialBuilder) -> SequentialBuilder:
    b.bottleneck_residual_block(64, 64, 256, 1, "layer1_block1")
    b.bottleneck_residual_block(256, 64, 256, 1, "layer1_block2")
    b.bottleneck_residual_block(256, 64, 256, 1, "layer1_block3")
    b.bottleneck_residual_block(256, 128, 512, 2, "layer2_block1")
    for i in range(2, 5):
        b.bottleneck_residual_block(512, 128, 512, 1, f"layer2_block{i}")
    b.bottleneck_residual_block(512, 256, 1024, 2, "layer3_block1")
    for i in range(2, 7):
        b.bottleneck_residual_block(1024, 256, 1024, 1, f"layer3_block{i}")
    b.bottleneck_residual_block(1024, 512, 2048, 2, "layer4_block1")
    for i in range(2, 4):
        b.bottleneck_residual_block(2048, 512, 2048, 1, f"layer4_block{i}")
    return b


def create_resnet50_cifar10() -> Sequential:
    b = (SequentialBuilder("ResNet-50-CIFAR10").input([3, 32, 32])
         .conv2d(64, 3, 3, 1, 1, 1, 1, True, "conv1").batchnorm(1e-5, 0.1, True, "bn1").activation("relu", "relu1"))
    return _resnet50_body(b).flatten("flatten").dense(10, True, "fc").build()


def create_resnet9_tiny_imagenet() -> Sequential:
    return (SequentialBuilder("ResNet-9-Tiny-ImageNet").input([3, 64, 64])
            .conv2d(64, 3, 3, 1, 1, 1, 1, False, "conv1").batchnorm(1e-5, 0.1, True, "bn1").activation("relu", "relu1")
            .conv2d(128, 3, 3, 1, 1, 1, 1, False, "conv2").batchnorm(1e-5, 0.1, True, "bn2").activation("relu", "relu2")
            .maxpool2d(2, 2, 2, 2, 0, 0, "pool1").basic_residual_block(128, 128, 1, "res1")
            .conv2d(256, 3, 3, 1, 1, 1, 1, False, "conv3").batchnorm(1e-5, 0.1, True, "bn3").activation("relu", "relu3")
            .maxpool2d(2, 2, 2, 2, 0, 0, "pool2").basic_residual_block(256, 256, 1, "res2")
            .conv2d(512, 3, 3, 1, 1, 1, 1, False, "conv4").batchnorm(1e-5, 0.1, True, "bn4").activation("relu", "relu4")
            .maxpool2d(2, 2, 2, 2, 0, 0, "pool3").basic_residual_block(512, 512, 1, "res3")
            .avgpool2d(4, 4, 1, 1, 0, 0, "avgpool").flatten("flatten").dense(200, True, "fc").build())


def create_cnn_tiny_imagenet() -> Sequential:
    b = _vgg_body(SequentialBuilder("sequential").input([3, 64, 64]))
    return b.dense(1024, True, "fc0").activation("relu", "relu10").dense(200, True, "fc1").build()


def create_resnet18_tiny_imagenet() -> Sequential:
    """Headline model (example_models.hpp:306-331): ~11.3 M params, ~1.08 GFLOP/sample fwd."""
    return (SequentialBuilder("ResNet-18-Tiny-ImageNet").input([3, 64, 64])
            .conv2d(32, 3, 3, 1, 1, 1, 1, False, "conv1").batchnorm(1e-3, 0.1, True, "bn1")
            .activation("relu", "relu1").maxpool2d(2, 2, 2, 2, 0, 0, "maxpool")
            .basic_residual_block(32, 64, 1, "layer1_block1").basic_residual_block(64, 64, 1, "layer1_block2")
            .basic_residual_block(64, 128, 2, "layer2_block1").basic_residual_block(128, 128, 1, "layer2_block2")
            .basic_residual_block(128, 256, 2, "layer3_block1").basic_residual_block(256, 256, 1, "layer3_block2")
            .basic_residual_block(256, 512, 2, "layer4_block1").basic_residual_block(512, 512, 1, "layer4_block2")
            .avgpool2d(4, 4, 1, 1, 0, 0, "avgpool").flatten("flatten").dense(200, True, "fc").build())


def create_resnet34_tiny_imagenet() -> Sequential:
    b = (SequentialBuilder("ResNet-34-Tiny-ImageNet").input([3, 64, 64])
         .conv2d(32, 3, 3, 1, 1, 1, 1, False, "conv1").batchnorm(1e-3, 0.1, True, "bn1")
         .activation("relu", "relu1").maxpool2d(2, 2, 2, 2, 0, 0, "maxpool"))
    b.basic_residual_block(32, 64, 1, "layer1_block1")
    for i in range(2, 4):
        b.basic_residual_block(64, 64, 1, f"layer1_block{i}")
    b.basic_residual_block(64, 128, 2, "layer2_block1")
    for i in range(2, 5):
        b.basic_residual_block(128, 128, 1, f"layer2_block{i}")
    b.basic_residual_block(128, 256, 2, "layer3_block1")
    for i in range(2, 7):
        b.basic_residual_block(256, 256, 1, f"layer3_block{i}")
    b.basic_residual_block(256, 512, 2, "layer4_block1")
    for i in range(2, 4):
        b.basic_residual_block(512, 512, 1, f"layer4_block{i}")
    return b.avgpool2d(4, 4, 1, 1, 0, 0, "avgpool").flatten("flatten").dense(200, True, "fc").build()


def create_resnet50_tiny_imagenet() -> Sequential:
    b = (SequentialBuilder("ResNet-50-Tiny-ImageNet").input([3, 64, 64])
         .conv2d(64, 3, 3, 1, 1, 1, 1, True, "conv1").batchnorm(1e-5, 0.1, True, "bn1")
         .activation("relu", "relu1").maxpool2d(3, 3, 2, 2, 1, 1, "maxpool"))
    return _resnet50_body(b).avgpool2d(4, 4, 1, 1, 0, 0, "avgpool").flatten("flatten").dense(200, True, "fc").build()


def create_resnet50_imagenet() -> Sequential:
    b = (SequentialBuilder("ResNet-50-ImageNet").input([3, 224, 224])
         .conv2d(64, 7, 7, 2, 2, 3, 3, True, "conv1").batchnorm(1e-5, 0.1, True, "bn1")
         .activation("relu", "relu1").maxpool2d(3, 3, 2, 2, 1, 1, "maxpool"))
    return _resnet50_body(b).avgpool2d(7, 7, 1, 1, 0, 0, "avgpool").flatten("flatten").dense(1000, True, "fc").build()


# MobileNetV1 body: (pointwise output channels, depthwise stride) of the 13 separable blocks
_MOBILENET_V1 = ((64, 1), (128, 2), (128, 1), (256, 2), (256, 1), (512, 2), (512, 1), (512, 1), (512, 1), (512, 1),
                 (512, 1), (1024, 2), (1024, 1))


def _mobilenet_v1(name, hw, classes) -> Sequential:
    """Stride-1 stem (the inputs are small; it rides the RGB stem kernel), 13 depthwise-separable
    blocks dw3x3 -> BN -> ReLU -> 1x1 -> BN -> ReLU, global average pool, classifier. Layer names
    and order match dcnn::create_model (train.cpp), so checkpoints interchange."""
    b = (SequentialBuilder(name).input([3, hw, hw])
         .conv2d(32, 3, 3, 1, 1, 1, 1, False, "conv1").batchnorm(1e-5, 0.1, True, "bn1").activation("relu", "relu1"))
    for i, (co, s) in enumerate(_MOBILENET_V1, 1):
        (b.depthwise_conv2d(3, 3, s, s, 1, 1, False, f"dw{i}").batchnorm(1e-5, 0.1, True, f"dw{i}_bn")
         .activation("relu", f"dw{i}_relu")
         .conv2d(co, 1, 1, 1, 1, 0, 0, False, f"pw{i}").batchnorm(1e-5, 0.1, True, f"pw{i}_bn")
         .activation("relu", f"pw{i}_relu"))
        hw = (hw + 2 - 3) // s + 1
    return b.avgpool2d(hw, hw, 1, 1, 0, 0, "avgpool").flatten("flatten").dense(classes, True, "fc").build()


def create_mobilenet_v1_cifar10() -> Sequential:
    return _mobilenet_v1("MobileNetV1-CIFAR10", 32, 10)


def create_mobilenet_v1_tiny_imagenet() -> Sequential:
    return _mobilenet_v1("MobileNetV1-Tiny-ImageNet", 64, 200)


# ResNeXt 32x4d: (grouped width, output width) per stage; the grouped 3x3 has 32 groups
_RESNEXT_WIDTHS = ((128, 256), (256, 512), (512, 1024), (1024, 2048))


def _resnext_body(b: SequentialBuilder, blocks, groups=32) -> SequentialBuilder:
    """Stages of bottleneck blocks 1x1 -> grouped 3x3 -> 1x1 (stride on the grouped conv of each
    stage's first block but the first stage's). With 32 groups the four stages have 4, 8, 16 and 32
    channels per group."""
    cin = 64
    for s, (n, (mid, out)) in enumerate(zip(blocks, _RESNEXT_WIDTHS), 1):
        for i in range(1, n + 1):
            b.resnext_bottleneck_block(cin, mid, out, groups, 2 if (i == 1 and s > 1) else 1, f"layer{s}_block{i}")
            cin = out
    return b


def create_resnext50_32x4d_tiny_imagenet() -> Sequential:
    b = (SequentialBuilder("ResNeXt-50-32x4d-Tiny-ImageNet").input([3, 64, 64])
         .conv2d(64, 3, 3, 1, 1, 1, 1, True, "conv1").batchnorm(1e-5, 0.1, True, "bn1")
         .activation("relu", "relu1").maxpool2d(3, 3, 2, 2, 1, 1, "maxpool"))
    return (_resnext_body(b, (3, 4, 6, 3)).avgpool2d(4, 4, 1, 1, 0, 0, "avgpool").flatten("flatten")
            .dense(200, True, "fc").build())


def create_resnext26_32x4d_cifar10() -> Sequential:
    b = (SequentialBuilder("ResNeXt-26-32x4d-CIFAR10").input([3, 32, 32])
         .conv2d(64, 3, 3, 1, 1, 1, 1, False, "conv1").batchnorm(1e-5, 0.1, True, "bn1").activation("relu", "relu1"))
    return (_resnext_body(b, (2, 2, 2, 2)).avgpool2d(4, 4, 1, 1, 0, 0, "avgpool").flatten("flatten")
            .dense(10, True, "fc").build())


def _convnext(name, hw, patch, depths, widths, classes, drop_path_rate=0.0) -> Sequential:
    """ConvNeXt (Liu et al. 2022): a patchify stem (patch x patch conv, stride = patch) + LayerNorm,
    four stages of ConvNeXt blocks with LayerNorm + 2x2 / stride-2 conv transitions, then average
    pool -> LayerNorm -> dense. Every bias is on. ``drop_path_rate``: stochastic depth, rising
    linearly over all blocks in order (block i of L gets rate * i / (L - 1); a block at rate 0 gets
    no DropPath layer, so rate 0 is exactly the model without it)."""
    if not 0.0 <= drop_path_rate < 1.0:
        raise ValueError(f"drop_path_rate must be in [0, 1), got {drop_path_rate}")
    total, k = sum(depths), 0
    b = (SequentialBuilder(name).input([3, hw, hw])
         .conv2d(widths[0], patch, patch, patch, patch, 0, 0, True, "stem_conv").layernorm(1e-6, True, "stem_ln"))
    for s, (n, w) in enumerate(zip(depths, widths), 1):
        if s > 1:
            b.convnext_downsample(w, f"down{s}")
        for i in range(1, n + 1):
            b.convnext_block(w, 1e-6, f"stage{s}_block{i}", drop_path_rate * k / max(total - 1, 1))
            k += 1
    m = b.get_current_shape()[2]
    return (b.avgpool2d(m, m, 1, 1, 0, 0, "avgpool").layernorm(1e-6, True, "head_ln").flatten("flatten")
            .dense(classes, True, "fc").build())


def create_convnext_pico_cifar10(drop_path_rate: float = 0.0) -> Sequential:
    return _convnext("ConvNeXt-Pico-CIFAR10", 32, 2, (2, 2, 6, 2), (64, 128, 256, 512), 10, drop_path_rate)


def create_convnext_tiny_tiny_imagenet(drop_path_rate: float = 0.0) -> Sequential:
    return _convnext("ConvNeXt-T-Tiny-ImageNet", 64, 4, (3, 3, 9, 3), (96, 192, 384, 768), 200, drop_path_rate)


MODELS = {
    "mnist_cnn": create_mnist_trainer,
    "cifar10_cnn_v1": create_cifar10_trainer_v1,
    "cifar10_cnn_v2": create_cifar10_trainer_v2,
    "resnet9_cifar10": create_resnet9_cifar10,
    "resnet18_cifar10": create_resnet18_cifar10,
    "resnet20_cifar10": create_resnet20_cifar10,
    "resnet50_cifar10": create_resnet50_cifar10,
    "resnet9_tiny_imagenet": create_resnet9_tiny_imagenet,
    "cnn_tiny_imagenet": create_cnn_tiny_imagenet,
    "resnet18_tiny_imagenet": create_resnet18_tiny_imagenet,
    "resnet34_tiny_imagenet": create_resnet34_tiny_imagenet,
    "resnet50_tiny_imagenet": create_resnet50_tiny_imagenet,
    "resnet50_imagenet": create_resnet50_imagenet,
    "mobilenet_v1_cifar10": create_mobilenet_v1_cifar10,
    "mobilenet_v1_tiny_imagenet": create_mobilenet_v1_tiny_imagenet,
    "resnext50_32x4d_tiny_imagenet": create_resnext50_32x4d_tiny_imagenet,
    "resnext26_32x4d_cifar10": create_resnext26_32x4d_cifar10,
    "convnext_pico_cifar10": create_convnext_pico_cifar10,
    "convnext_tiny_tiny_imagenet": create_convnext_tiny_tiny_imagenet,
}

INPUT_SHAPES = {
    "mnist_cnn": (1, 28, 28), "cifar10_cnn_v1": (3, 32, 32), "cifar10_cnn_v2": (3, 32, 32),
    "resnet9_cifar10": (3, 32, 32), "resnet18_cifar10": (3, 32, 32), "resnet20_cifar10": (3, 32, 32),
    "resnet50_cifar10": (3, 32, 32), "resnet9_tiny_imagenet": (3, 64, 64), "cnn_tiny_imagenet": (3, 64, 64),
    "resnet18_tiny_imagenet": (3, 64, 64), "resnet34_tiny_imagenet": (3, 64, 64),
    "resnet50_tiny_imagenet": (3, 64, 64), "resnet50_imagenet": (3, 224, 224),
    "mobilenet_v1_cifar10": (3, 32, 32), "mobilenet_v1_tiny_imagenet": (3, 64, 64),
    "resnext50_32x4d_tiny_imagenet": (3, 64, 64), "resnext26_32x4d_cifar10": (3, 32, 32),
    "convnext_pico_cifar10": (3, 32, 32), "convnext_tiny_tiny_imagenet": (3, 64, 64),
}

NUM_CLASSES = {k: (10 if ("cifar" in k or "mnist" in k) else (1000 if k == "resnet50_imagenet" else 200))
               for k in MODELS}


def create_model(name: str, **kwargs) -> Sequential:
    """``kwargs`` go to the model's builder (``drop_path_rate`` for the ConvNeXt models)."""
    if name not in MODELS:
        raise KeyError(f"unknown model {name!r}; available: {sorted(MODELS)}")
    return MODELS[name](**kwargs)
