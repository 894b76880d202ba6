#!/usr/bin/env python3
"""Real-data feeding at GPU speed: decode, host loader, HBM-resident loader and end-to-end training.

Builds a synthetic Tiny-ImageNet directory (PIL-written 64x64 JPEGs in the reference's layout:
wnids.txt, words.txt, train/<wnid>/images/*.JPEG, val/images + val_annotations.txt), then times:

1. ``decode``: the native JPEG decoder over the directory (``TinyImageNetDataLoader.load_data``,
   all host threads) — images/s and images/s per host core;
2. ``host_loader``: the host path — native gather + host augmentation (crop + flip + normalise) +
   pinned staging + H2D on a side stream (``BaseDataLoader`` with ``device="cuda"``);
3. ``device_loader``: the HBM-resident path — one ``augment_batch`` launch per batch
   (``DeviceDataLoader``), timed with device synchronisation;
4. ``train``: ResNet-18-tiny training steps (hipGraph, Adam) fed by the device loader, against the
   same steps on a fixed synthetic batch (``bench.py``'s loop) — the ratio is the share of the
   GPU step rate that real data keeps.

  python benchmarks/loader_bench.py --images-per-class 50 --batch 256 --steps 40

``--mix`` times Mixup / CutMix instead (synthetic 3x64x64 uint8 images in HBM, no JPEG directory):
``mix_batch`` alone against a device-to-device copy of the same bytes, batch assembly with and without
the mixer, the loss kernel (soft_crossentropy on a dense target against softmax_crossentropy on
labels) and ResNet-18-tiny training steps fed by the HBM-resident loader with mixer +
soft_crossentropy(0.1) against labels + softmax_crossentropy, in alternating rounds.

  python benchmarks/loader_bench.py --mix --batch 256 --steps 200 --rounds 5
Reference: include/data_loading/tiny_imagenet_data_loader.hpp:278-560, include/nn/train.hpp:108-147.
"""
import argparse
import io
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_dataset(root, classes, per_class, val_per_class, seed=0):
    from PIL import Image
    g = np.random.default_rng(seed)
    wnids = [f"n{10000000 + i:08d}" for i in range(classes)]
    os.makedirs(root, exist_ok=True)
    with open(os.path.join(root, "wnids.txt"), "w") as f:
        f.write("\n".join(wnids) + "\n")
    with open(os.path.join(root, "words.txt"), "w") as f:
        f.write("\n".join(f"{w}\tclass {i}" for i, w in enumerate(wnids)) + "\n")
    base = g.integers(0, 256, (classes, 8, 8, 3))

    def img(c):
        # a class-coloured smooth pattern + noise (compressible like a photo, not like white noise)
        up = np.kron(base[c], np.ones((8, 8, 1)))
        return np.clip(up + g.normal(0, 20, up.shape), 0, 255).astype(np.uint8)

    for c, w in enumerate(wnids):
        d = os.path.join(root, "train", w, "images")
        os.makedirs(d, exist_ok=True)
        for i in range(per_class):
            Image.fromarray(img(c)).save(os.path.join(d, f"{w}_{i}.JPEG"), "JPEG", quality=90)
    vd = os.path.join(root, "val", "images")
    os.makedirs(vd, exist_ok=True)
    with open(os.path.join(root, "val", "val_annotations.txt"), "w") as f:
        k = 0
        for c, w in enumerate(wnids):
            for i in range(val_per_class):
                name = f"val_{k}.JPEG"
                Image.fromarray(img(c)).save(os.path.join(vd, name), "JPEG", quality=90)
                f.write(f"{name}\t{w}\t0\t0\t63\t63\n")
                k += 1
    return classes * per_class


def _graph_us(fns, replays=20):
    """Mean microseconds of one call: every ``fn`` of ``fns`` is captured once into one graph (side-stream
    warm-up first, as runtime/step.py captures), the graph is replayed ``replays`` times between two
    device events. Replays take the host (Python, the launch path) out of the figure; ``fns`` that walk
    over more memory than the 256 MB last-level cache keep it out too."""
    from dcnn_amd.runtime.capture import capture_guard
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for fn in fns[:2]:
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with capture_guard(), torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
        keep = [fn() for fn in fns]  # (outputs stay alive: every node keeps its own buffers)
    for _ in range(3):
        g.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(replays):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    del keep
    return e0.elapsed_time(e1) * 1e3 / (replays * len(fns))


def mix_bench(a):
    from dcnn_amd.data import AugmentationBuilder, BatchMixer, DeviceDataLoader
    from dcnn_amd.models import create_model
    from dcnn_amd.nn import Adam, LossFactory
    from dcnn_amd.ops import hip
    from dcnn_amd.runtime.step import TrainStep
    B, C, H, W, K = a.batch, 3, 64, 64, a.classes
    g = torch.Generator().manual_seed(0)
    lab = torch.randint(0, K, (B,), generator=g).cuda()
    tgt = torch.empty(B, K, device="cuda")
    nbytes = B * C * H * W * 4

    # ---- 1. mix_batch alone against a copy of the same bytes: graph replays over `nb` distinct batches
    # (more than the last-level cache holds), alternating rounds
    nb = max(2, (768 << 20) // nbytes)
    xs = [torch.randn(B, C, H, W, generator=g).cuda() for _ in range(4)]
    xs = [xs[i % 4].clone() for i in range(nb)]
    ds = [torch.empty_like(t) for t in xs]
    bh = bw = H // 2
    box = (H // 4, H // 4 + bh, W // 4, W // 4 + bw)
    nbox = B * C * bh * bw
    bsrc = [torch.empty(nbox, device="cuda") for _ in range(nb)]
    bdst = [torch.empty(nbox, device="cuda") for _ in range(nb)]
    calls = {
        "mixup": [lambda t=t: hip.mix_batch(t, lab, tgt, 1, 0.5, (0, 0, 0, 0), K) for t in xs],
        "copy": [lambda t=t, d=d: d.copy_(t) for t, d in zip(xs, ds)],
        "cutmix": [lambda t=t: hip.mix_batch(t, lab, tgt, 2, 0.75, box, K) for t in xs],
        "copy_box": [lambda t=t, d=d: d.copy_(t) for t, d in zip(bsrc, bdst)],
        "mode0_target_only": [lambda t=t: hip.mix_batch(t, lab, tgt, 0, 1.0, (0, 0, 0, 0), K) for t in xs],
    }
    rows = {k: [] for k in calls}
    for _ in range(a.rounds):
        for k, fns in calls.items():
            rows[k].append(_graph_us(fns))
    med = {k: float(np.median(v)) for k, v in rows.items()}
    print(json.dumps({"phase": "mix_batch", "batch": B, "row": [C, H, W], "classes": K, "batch_bytes": nbytes,
                      "distinct_batches": nb, "box": box, "box_bytes": nbox * 4, "rounds": a.rounds,
                      "timing": "graph replays, device events, per call",
                      "us": {k: [round(t, 2) for t in v] for k, v in rows.items()},
                      "median_us": {k: round(t, 2) for k, t in med.items()},
                      "mixup_gbps_read_plus_write": round(2 * nbytes / med["mixup"] / 1e3, 1),
                      "copy_gbps_read_plus_write": round(2 * nbytes / med["copy"] / 1e3, 1),
                      "cutmix_gbps_read_plus_write": round(2 * nbox * 4 / med["cutmix"] / 1e3, 1),
                      "copy_box_gbps_read_plus_write": round(2 * nbox * 4 / med["copy_box"] / 1e3, 1),
                      "copy_over_mixup": round(med["copy"] / med["mixup"], 3),
                      "copy_box_over_cutmix": round(med["copy_box"] / med["cutmix"], 3)}), flush=True)
    del xs, ds, bsrc, bdst, calls

    # ---- 2. the loss kernel: kind 6 on a dense target against kind 1 on labels (graph replays of 64 calls)
    logits = torch.randn(B, K, generator=g).cuda().to(torch.bfloat16)
    dense = torch.softmax(torch.randn(B, K, generator=g), 1).cuda()
    calls = {
        "soft_dense": [lambda: hip.loss_fused(logits, dense, None, "soft_crossentropy", 0.1)] * 64,
        "softmax_labels": [lambda: hip.loss_fused(logits, None, lab, "softmax_crossentropy")] * 64,
        "soft_labels": [lambda: hip.loss_fused(logits, None, lab, "soft_crossentropy", 0.1)] * 64,
    }
    rows = {k: [] for k in calls}
    for _ in range(a.rounds):
        for k, fns in calls.items():
            rows[k].append(_graph_us(fns))
    print(json.dumps({"phase": "loss_kernel", "N": B, "C": K, "dtype": "bf16", "rounds": a.rounds,
                      "timing": "graph replays of 64 back-to-back launches, device events, per launch",
                      "us": {k: [round(t, 2) for t in v] for k, v in rows.items()},
                      "median_us": {k: round(float(np.median(v)), 2) for k, v in rows.items()}}), flush=True)

    # ---- 3. batch assembly with and without the mixer
    n = max(B * 8, 4096)
    rng = np.random.default_rng(0)
    data = (rng.integers(0, 256, (n, C, H, W), dtype=np.uint8) / np.float32(255)).astype(np.float32)
    labels = rng.integers(0, K, n)

    def loader():
        ld = DeviceDataLoader(data=data, labels=labels, num_classes=K, batch_size=B, shuffle=True, seed=1,
                              drop_last=True, storage="u8")
        ld.set_augmentation(AugmentationBuilder().random_crop(0.5, 4).horizontal_flip(0.5).normalize().build())
        ld.reset()
        return ld

    def batch_of(ld):
        b = ld.get_next_batch()
        if b is None:
            ld.reset()
            b = ld.get_next_batch()
        return b

    plain, mixed = loader(), loader()
    mixed.set_mixer(BatchMixer(K, seed=1))
    rows = {"plain": [], "mixed": []}
    for _ in range(a.rounds):
        for name, ld in (("plain", plain), ("mixed", mixed)):
            for _ in range(5):
                batch_of(ld)
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(100):
                batch_of(ld)
            torch.cuda.synchronize()
            rows[name].append(100 * B / (time.perf_counter() - t))
    print(json.dumps({"phase": "assembly", "batch": B, "rounds": a.rounds,
                      "images_per_sec": {k: [round(v) for v in r] for k, r in rows.items()},
                      "median_images_per_sec": {k: round(float(np.median(r))) for k, r in rows.items()}}), flush=True)

    # ---- 4. training steps fed by the HBM-resident loader, alternating rounds
    def trainer(soft):
        m = create_model("resnet18_tiny_imagenet")
        m.set_seed(1)
        m.set_device("GPU:0")
        m.initialize()
        m.set_first_layer_input_grad(False)
        opt = Adam(1e-3)
        opt.attach(m)
        loss = LossFactory.create("soft_crossentropy", label_smoothing=0.1) if soft else \
            LossFactory.create("softmax_crossentropy")
        return TrainStep(m, loss, opt, use_graph=True)

    runs = {"labels_softmax_ce": (trainer(False), plain), "mixer_soft_ce": (trainer(True), mixed)}
    for st, ld in runs.values():
        for _ in range(10):
            st(*batch_of(ld))
    torch.cuda.synchronize()
    rows = {k: [] for k in runs}
    for _ in range(a.rounds):
        for name, (st, ld) in runs.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(a.steps):
                st(*batch_of(ld))
            torch.cuda.synchronize()
            rows[name].append((time.perf_counter() - t) / a.steps * 1e3)
    mean = {k: float(np.mean(v)) for k, v in rows.items()}
    print(json.dumps({"phase": "train_mix", "model": "resnet18_tiny_imagenet", "batch": B, "steps": a.steps,
                      "rounds": a.rounds, "ms_per_step": {k: [round(v, 4) for v in r] for k, r in rows.items()},
                      "mean_ms_per_step": {k: round(v, 4) for k, v in mean.items()},
                      "spread_ms": {k: round(max(r) - min(r), 4) for k, r in rows.items()},
                      "difference_percent": round(100 * (mean["mixer_soft_ce"] / mean["labels_softmax_ce"] - 1), 2),
                      "final_loss": {k: round(float(st.last_loss), 4) for k, (st, _) in runs.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", type=int, default=200)
    ap.add_argument("--images-per-class", type=int, default=50)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--root", default="")
    ap.add_argument("--mix", action="store_true", help="time Mixup / CutMix and the soft-target loss instead")
    ap.add_argument("--rounds", type=int, default=5, help="--mix: alternating rounds per comparison")
    a = ap.parse_args()
    if a.mix:
        return mix_bench(a)
    from dcnn_amd.data import AugmentationBuilder, TinyImageNetDataLoader, to_device_loader
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    root = a.root or tempfile.mkdtemp(prefix="tinyimg_")
    t0 = time.perf_counter()
    n = make_dataset(root, a.classes, a.images_per_class, 2)
    print(json.dumps({"phase": "make_dataset", "images": n, "s": round(time.perf_counter() - t0, 2)}), flush=True)

    tr = TinyImageNetDataLoader(batch_size=a.batch, shuffle=True, seed=1, device="cuda")
    t0 = time.perf_counter()
    tr.load_data(root, True)
    dt = time.perf_counter() - t0
    print(json.dumps({"phase": "decode", "images": tr.size(), "images_per_sec": round(tr.size() / dt),
                      "host_cores": cores, "images_per_sec_per_core": round(tr.size() / dt / cores),
                      "failures": tr.decode_failures}), flush=True)
    aug = AugmentationBuilder().random_crop(0.5, 4).horizontal_flip(0.5).normalize().build()
    tr.set_augmentation(aug)

    def time_loader(ld, batches):
        ld.reset()
        got = 0
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(batches):
            b = ld.get_next_batch()
            if b is None:
                ld.reset()
                b = ld.get_next_batch()
            got += b[0].shape[0]
        torch.cuda.synchronize()
        return got / (time.perf_counter() - t)

    nb = max(4, min(a.steps, tr.num_batches() - 1))
    ips = time_loader(tr, nb)
    print(json.dumps({"phase": "host_loader", "images_per_sec": round(ips), "host_cores": cores,
                      "images_per_sec_per_core": round(ips / cores),
                      "path": "native gather + host augmentation + pinned staging + H2D"}), flush=True)
    dl = to_device_loader(tr)
    ips_d = time_loader(dl, nb)
    print(json.dumps({"phase": "device_loader", "images_per_sec": round(ips_d), "storage": dl.storage,
                      "device_bytes": dl._data.numel() * dl._data.element_size(),
                      "path": "HBM-resident uint8 + augment_batch kernel"}), flush=True)

    # ---- end to end: training steps fed by the device loader vs a fixed synthetic batch
    from dcnn_amd.models import create_model
    from dcnn_amd.nn import Adam, LossFactory
    from dcnn_amd.runtime.step import TrainStep
    m = create_model("resnet18_tiny_imagenet")
    m.set_seed(1)
    m.set_device("GPU:0")
    m.initialize()
    m.set_first_layer_input_grad(False)
    opt = Adam(1e-3)
    opt.attach(m)
    st = TrainStep(m, LossFactory.create("softmax_crossentropy"), opt, use_graph=True)
    dl.drop_last = True
    dl.reset()

    def batch():
        b = dl.get_next_batch()
        if b is None:
            dl.reset()
            b = dl.get_next_batch()
        return b

    for _ in range(5):
        st(*batch())
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(a.steps):
        st(*batch())
    torch.cuda.synchronize()
    real = a.batch * a.steps / (time.perf_counter() - t)
    x0, y0 = batch()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(a.steps):
        st(x0, y0)
    torch.cuda.synchronize()
    synth = a.batch * a.steps / (time.perf_counter() - t)
    print(json.dumps({"phase": "train", "model": "resnet18_tiny_imagenet", "batch": a.batch,
                      "images_per_sec_device_loader": round(real), "images_per_sec_fixed_batch": round(synth),
                      "ratio": round(real / synth, 3), "final_loss": round(float(st.last_loss), 4)}), flush=True)


if __name__ == "__main__":
    main()
