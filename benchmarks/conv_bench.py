#!/usr/bin/env python3
"""Per-shape microbenchmark of the implicit-GEMM conv kernels (fwd / dgrad / wgrad) on the
ResNet-18-tiny layer shapes. Reports device time per call and achieved TFLOP/s.

  python benchmarks/conv_bench.py --batch 256 [--only fwd|dgrad|wgrad] [--iters 20]

--depthwise: the depthwise-conv streaming kernels (dwconv.hip) at the MobileNetV1-Tiny-ImageNet
shapes instead — per pass the device time, the compulsory GB/s, a plain device copy moving the
same number of bytes, PyTorch's F.conv2d(groups=C) passes (bf16 channels_last) and, with --step,
the captured training step of mobilenet_v1_tiny_imagenet on the Python engine.

--grouped: the grouped-conv MFMA kernels (gconv.hip) at the ResNeXt-50-32x4d-Tiny-ImageNet shapes,
same method — against a same-bytes copy, PyTorch's F.conv2d(groups=32) passes and the project's own
dense conv at the same channel counts, with the percentage of the bf16 MFMA peak the issued FLOPs
reach and, with --step, the captured training step of resnext50_32x4d_tiny_imagenet.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (name, Ci, H, W, Co, k, s, p)
SHAPES = [
    ("stem", 3, 64, 64, 32, 3, 1, 1),
    ("l1.b1c1", 32, 32, 32, 64, 3, 1, 1),
    ("l1.c", 64, 32, 32, 64, 3, 1, 1),
    ("l1.proj", 32, 32, 32, 64, 1, 1, 0),
    ("l2.b1c1", 64, 32, 32, 128, 3, 2, 1),
    ("l2.c", 128, 16, 16, 128, 3, 1, 1),
    ("l2.proj", 64, 32, 32, 128, 1, 2, 0),
    ("l3.b1c1", 128, 16, 16, 256, 3, 2, 1),
    ("l3.c", 256, 8, 8, 256, 3, 1, 1),
    ("l3.proj", 128, 16, 16, 256, 1, 2, 0),
    ("l4.b1c1", 256, 8, 8, 512, 3, 2, 1),
    ("l4.c", 512, 4, 4, 512, 3, 1, 1),
    ("l4.proj", 256, 8, 8, 512, 1, 2, 0),
]

# ResNet-50-tiny bottleneck shapes (64x64 input, stride-2 max-pool stem: layer 1 at 32x32);
# --set r50 (include/nn/example_models.hpp:369-402 block structure)
SHAPES_R50 = [
    ("r1.c1a", 64, 32, 32, 64, 1, 1, 0),     # layer1_block1 1x1 reduce (64 in)
    ("r1.c1", 256, 32, 32, 64, 1, 1, 0),     # layer1 1x1 reduce
    ("r1.c2", 64, 32, 32, 64, 3, 1, 1),      # layer1 3x3
    ("r1.c3", 64, 32, 32, 256, 1, 1, 0),     # layer1 1x1 expand
    ("r2.c1", 512, 16, 16, 128, 1, 1, 0),
    ("r2.c2", 128, 16, 16, 128, 3, 1, 1),
    ("r2.c3", 128, 16, 16, 512, 1, 1, 0),
    ("r2.s2", 128, 32, 32, 128, 3, 2, 1),    # layer2_block1 strided 3x3
    ("r2.proj", 256, 32, 32, 512, 1, 2, 0),
    ("r3.c1", 1024, 8, 8, 256, 1, 1, 0),
    ("r3.c2", 256, 8, 8, 256, 3, 1, 1),
    ("r3.c3", 256, 8, 8, 1024, 1, 1, 0),
    ("r4.c1", 2048, 4, 4, 512, 1, 1, 0),
    ("r4.c2", 512, 4, 4, 512, 3, 1, 1),
    ("r4.c3", 512, 4, 4, 2048, 1, 1, 0),
]


# every distinct depthwise (C, H, W, stride) of mobilenet_v1_tiny_imagenet (3x3, pad 1)
SHAPES_DW = [(32, 64, 64, 1), (64, 64, 64, 2), (128, 32, 32, 1), (128, 32, 32, 2), (256, 16, 16, 1), (256, 16, 16, 2),
             (512, 8, 8, 1), (512, 8, 8, 2), (1024, 4, 4, 1)]


def _time_graph(fn, iters, reps):
    """Median / min / max device microseconds per call over `reps` replays of a graph of `iters`
    calls (no host launch overhead); eager launches if the calls cannot be captured."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    try:
        g = torch.cuda.CUDAGraph()
        s_ = torch.cuda.Stream()
        s_.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s_):
            with torch.cuda.graph(g, stream=s_):
                for _ in range(iters):
                    fn()
        torch.cuda.current_stream().wait_stream(s_)
        run, mode = g.replay, "graph"
    except Exception:  # noqa: BLE001 (a library call that allocates or synchronises inside the capture)
        torch.cuda.synchronize()

        def run():
            for _ in range(iters):
                fn()
        mode = "eager"
    run()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1000 / iters)
    us.sort()
    return us[len(us) // 2], us[0], us[-1], mode


def depthwise_main(a):
    import json
    import torch.nn.functional as F
    from dcnn_amd.ops import hip
    CL = torch.channels_last
    N = a.batch
    rows = []
    print(f"{'shape':<18}{'op':<7}{'us':>9}{'min':>9}{'max':>9}{'GB/s':>8}{'copy us':>9}{'% copy':>8}{'torch us':>10}"
          f"{'torch/ours':>11}")
    for (C, H, W, s) in SHAPES_DW:
        OH, OW = (H + 2 - 3) // s + 1, (W + 2 - 3) // s + 1
        x = torch.randn(N, C, H, W, device="cuda").bfloat16().contiguous(memory_format=CL)
        w = (torch.randn(C, 1, 3, 3, device="cuda") / 3).bfloat16()
        dy = torch.randn(N, C, OH, OW, device="cuda").bfloat16().contiguous(memory_format=CL)
        gw = torch.zeros(C, 1, 3, 3, device="cuda")
        xb, yb = 2.0 * N * H * W * C, 2.0 * N * OH * OW * C
        # compulsory bytes: each activation read or written once (weights and slabs are < 1 %)
        hbm = {"fwd": xb + yb, "dgrad": xb + yb, "wgrad": xb + yb}
        ops = {"fwd": lambda: hip.dwconv2d_fwd(x, w, None, (s, s), (1, 1)),
               "dgrad": lambda: hip.dwconv2d_dgrad(dy, w, tuple(x.shape), (s, s), (1, 1)),
               "wgrad": lambda: hip.dwconv2d_wgrad(dy, x, tuple(w.shape), (s, s), (1, 1), gw, None)}
        aten = torch.ops.aten.convolution_backward
        bwd = lambda mask: aten(dy, x, w, None, [s, s], [1, 1], [1, 1], False, [0, 0], C, mask)  # noqa: E731
        tops = {"fwd": lambda: F.conv2d(x, w, None, s, 1, groups=C),
                "dgrad": lambda: bwd([True, False, False]), "wgrad": lambda: bwd([False, True, False])}
        for op, fn in ops.items():
            if a.only and op != a.only:
                continue
            us, lo, hi, _ = _time_graph(fn, a.iters, a.reps)
            # a flat copy moving the same bytes (half of them read, half written)
            n = int(hbm[op] / 2) // 2
            src, dst = torch.empty(n, device="cuda", dtype=torch.bfloat16), torch.empty(n, device="cuda", dtype=torch.bfloat16)
            cus, _, _, _ = _time_graph(lambda: dst.copy_(src), a.iters, a.reps)
            del src, dst
            tus, tmode = float("nan"), "-"
            if a.torch_ref:
                tus, _, _, tmode = _time_graph(tops[op], a.iters, a.reps)
            r = dict(C=C, H=H, W=W, stride=s, op=op, us=us, us_min=lo, us_max=hi, gbs=hbm[op] / us / 1e3, copy_us=cus,
                     pct_copy=100.0 * cus / us, torch_us=tus, torch_mode=tmode, torch_over_ours=tus / us)
            rows.append(r)
            print(f"{f'c{C} {H}x{W} s{s}':<18}{op:<7}{us:9.1f}{lo:9.1f}{hi:9.1f}{r['gbs']:8.0f}{cus:9.1f}{r['pct_copy']:8.1f}"
                  f"{tus:10.1f}{tus / us:11.2f}", flush=True)
            if a.json:
                with open(a.json, "w") as f:
                    json.dump(dict(batch=N, iters=a.iters, reps=a.reps, rows=rows), f, indent=1)
    step = None
    if a.step:
        from dcnn_amd.models import create_model
        from dcnn_amd.nn import Adam, LossFactory
        from dcnn_amd.runtime.step import TrainStep
        m = create_model("mobilenet_v1_tiny_imagenet")
        m.set_seed(1)
        m.set_device("GPU:0")
        m.initialize()
        m.set_first_layer_input_grad(False)
        opt = Adam(1e-3)
        opt.attach(m)
        st = TrainStep(m, LossFactory.create("softmax_crossentropy"), opt, use_graph=True)
        xs = torch.randn(N, 3, 64, 64, device="cuda")
        ys = torch.randint(0, 200, (N,), device="cuda")
        for _ in range(6):
            st(xs, ys)
        torch.cuda.synchronize()
        ms = []
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(a.reps):
            e0.record()
            for _ in range(20):
                st(xs, ys)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / 20)
        ms.sort()
        step = dict(model="mobilenet_v1_tiny_imagenet", batch=N, graph=st.graphs is not None, ms=ms[len(ms) // 2],
                    ms_min=ms[0], ms_max=ms[-1], img_s=N * 1000.0 / ms[len(ms) // 2], loss=float(st.last_loss.item()))
        print("training step:", step, flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(batch=N, iters=a.iters, reps=a.reps, rows=rows, step=step), f, indent=1)


# every distinct grouped (C = Ci = Co, H, W, stride, layers of that shape) of
# resnext50_32x4d_tiny_imagenet (3x3, pad 1, 32 groups: 4, 8, 16 and 32 channels per group)
SHAPES_GC = [(128, 32, 32, 1, 3), (256, 32, 32, 2, 1), (256, 16, 16, 1, 3), (512, 16, 16, 2, 1), (512, 8, 8, 1, 5),
             (1024, 8, 8, 2, 1), (1024, 4, 4, 1, 2)]
GC_GROUPS = 32
MFMA_BF16_PEAK = 2.5e15  # dense bf16 FLOP/s of the chip (datasheet)


def _gc_issued_flops(N, C, G, H, W, OH, OW, T):
    """MFMA FLOPs the gconv.hip kernels issue (their tiling, bundle and zero-tap padding included)
    per pass, next to the useful 2 * pixels * C * (C / G) * T."""
    cg = C // G
    bundle = 1 if cg >= 16 else 16 // cg
    steps = -(-(T * -(-(bundle * cg) // 8)) // 4)          # 32-deep k-steps per 16-channel tile
    cpad = -(-C // 16) * 16
    fd = lambda pix: 2.0 * (-(-pix // 64) * 64) * cpad * 32 * steps  # noqa: E731
    nct = -(-(bundle * cg) // 16)
    wg = 2.0 * (-(-N * OH * OW // 32) * 32) * 16 * 16 * (cpad // 16) * nct * T
    return {"fwd": fd(N * OH * OW), "dgrad": fd(N * H * W), "wgrad": wg}


def grouped_main(a):
    import json
    import torch.nn.functional as F
    from dcnn_amd.ops import hip
    CL = torch.channels_last
    N, G = a.batch, GC_GROUPS
    rows = []
    print(f"{'shape':<18}{'op':<7}{'us':>9}{'min':>9}{'max':>9}{'copy us':>9}{'% copy':>8}{'% peak':>8}{'pad x':>7}"
          f"{'torch us':>10}{'torch/ours':>11}{'dense us':>10}{'dense/ours':>11}")
    for (C, H, W, s, count) in SHAPES_GC:
        OH, OW = (H + 2 - 3) // s + 1, (W + 2 - 3) // s + 1
        cg = C // G
        x = torch.randn(N, C, H, W, device="cuda").bfloat16().contiguous(memory_format=CL)
        w = (torch.randn(C, cg, 3, 3, device="cuda") / (9 * cg) ** 0.5).bfloat16().contiguous(memory_format=CL)
        dy = torch.randn(N, C, OH, OW, device="cuda").bfloat16().contiguous(memory_format=CL)
        gw = torch.zeros(C, cg, 3, 3, device="cuda").contiguous(memory_format=CL)
        # the project's dense conv at the same channel counts (G times the arithmetic and weight bytes)
        wd = (torch.randn(C, C, 3, 3, device="cuda") / (9 * C) ** 0.5).bfloat16().contiguous(memory_format=CL)
        wdt = hip.conv_weight_t(wd, dtype=torch.bfloat16)
        gwd = torch.zeros(C, C, 3, 3, device="cuda").contiguous(memory_format=CL)
        xb, yb = 2.0 * N * H * W * C, 2.0 * N * OH * OW * C
        # compulsory bytes: each activation read or written once (weights and slabs are < 1 %)
        hbm = {"fwd": xb + yb, "dgrad": xb + yb, "wgrad": xb + yb}
        useful = 2.0 * N * OH * OW * C * cg * 9
        issued = _gc_issued_flops(N, C, G, H, W, OH, OW, 9)
        ops = {"fwd": lambda: hip.gconv2d_fwd(x, w, None, (s, s), (1, 1), G),
               "dgrad": lambda: hip.gconv2d_dgrad(dy, w, tuple(x.shape), (s, s), (1, 1), G),
               "wgrad": lambda: hip.gconv2d_wgrad(dy, x, tuple(w.shape), (s, s), (1, 1), G, gw, None)}
        dops = {"fwd": lambda: hip.conv2d_fwd(x, wd, None, (s, s), (1, 1)),
                "dgrad": lambda: hip.conv2d_dgrad(dy, wdt, tuple(x.shape), (s, s), (1, 1)),
                "wgrad": lambda: hip.conv2d_wgrad(dy, x, tuple(wd.shape), (s, s), (1, 1), gwd, None)}
        aten = torch.ops.aten.convolution_backward
        bwd = lambda mask: aten(dy, x, w, None, [s, s], [1, 1], [1, 1], False, [0, 0], G, mask)  # noqa: E731
        tops = {"fwd": lambda: F.conv2d(x, w, None, s, 1, groups=G),
                "dgrad": lambda: bwd([True, False, False]), "wgrad": lambda: bwd([False, True, False])}
        for op, fn in ops.items():
            if a.only and op != a.only:
                continue
            us, lo, hi, _ = _time_graph(fn, a.iters, a.reps)
            # a flat copy moving the same bytes (half of them read, half written)
            n = int(hbm[op] / 2) // 2
            src, dst = torch.empty(n, device="cuda", dtype=torch.bfloat16), torch.empty(n, device="cuda", dtype=torch.bfloat16)
            cus, _, _, _ = _time_graph(lambda: dst.copy_(src), a.iters, a.reps)
            del src, dst
            dus, _, _, _ = _time_graph(dops[op], a.iters, a.reps)
            tus, tmode = float("nan"), "-"
            if a.torch_ref:
                tus, _, _, tmode = _time_graph(tops[op], a.iters, a.reps)
            r = dict(C=C, G=G, H=H, W=W, stride=s, layers=count, op=op, us=us, us_min=lo, us_max=hi, copy_us=cus,
                     pct_copy=100.0 * cus / us, issued_flops=issued[op], useful_flops=useful,
                     pct_peak=100.0 * issued[op] / (us * 1e-6) / MFMA_BF16_PEAK, torch_us=tus, torch_mode=tmode,
                     torch_over_ours=tus / us, dense_us=dus, dense_over_ours=dus / us)
            rows.append(r)
            print(f"{f'c{C} {H}x{W} s{s}':<18}{op:<7}{us:9.1f}{lo:9.1f}{hi:9.1f}{cus:9.1f}{r['pct_copy']:8.1f}"
                  f"{r['pct_peak']:8.2f}{issued[op] / useful:7.1f}{tus:10.1f}{tus / us:11.2f}{dus:10.1f}{dus / us:11.2f}",
                  flush=True)
            if a.json:
                with open(a.json, "w") as f:
                    json.dump(dict(batch=N, iters=a.iters, reps=a.reps, rows=rows), f, indent=1)
    step = None
    if a.step:
        from dcnn_amd.models import create_model
        from dcnn_amd.nn import Adam, LossFactory
        from dcnn_amd.runtime.step import TrainStep
        m = create_model("resnext50_32x4d_tiny_imagenet")
        m.set_seed(1)
        m.set_device("GPU:0")
        m.initialize()
        m.set_first_layer_input_grad(False)
        opt = Adam(1e-3)
        opt.attach(m)
        st = TrainStep(m, LossFactory.create("softmax_crossentropy"), opt, use_graph=True)
        xs = torch.randn(N, 3, 64, 64, device="cuda")
        ys = torch.randint(0, 200, (N,), device="cuda")
        for _ in range(6):
            st(xs, ys)
        torch.cuda.synchronize()
        ms = []
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(a.reps):
            e0.record()
            for _ in range(20):
                st(xs, ys)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / 20)
        ms.sort()
        # the grouped launches' share: the table's per-pass medians times the layers of each shape
        gc_ms = sum(r["us"] * r["layers"] for r in rows) / 1000.0
        step = dict(model="resnext50_32x4d_tiny_imagenet", batch=N, graph=st.graphs is not None,
                    ms=ms[len(ms) // 2], ms_min=ms[0], ms_max=ms[-1], img_s=N * 1000.0 / ms[len(ms) // 2],
                    loss=float(st.last_loss.item()), grouped_ms=gc_ms, grouped_share=gc_ms / ms[len(ms) // 2])
        print("training step:", step, flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(batch=N, iters=a.iters, reps=a.reps, rows=rows, step=step), f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", default="")
    ap.add_argument("--shapes", default="", help="comma-separated shape names (default: all)")
    ap.add_argument("--set", default="r18", choices=["r18", "r50"], help="ResNet-18-tiny or ResNet-50-tiny shapes")
    ap.add_argument("--v3", type=int, default=1, help="third-generation 3x3 halo conv (hconv3.hip) on/off")
    ap.add_argument("--eager", action="store_true", help="time eager launches instead of one hipGraph replay")
    ap.add_argument("--halo-1x1", type=int, default=1, help="K >= 1024 1x1 convs on the halo kernel (ops/fusion.py)")
    ap.add_argument("--torch-mm", action="store_true",
                    help="also time the 1x1 shapes' plain GEMMs on torch.mm (hipBLASLt; no fused statistics)")
    ap.add_argument("--hwgrad-s2", type=int, default=None, help="3x3 stride-2 wgrad on the stride-2 halo kernel (ops/fusion.py)")
    ap.add_argument("--split-target", type=int, default=None, help="hconv split-K workgroup target (tuning hook)")
    ap.add_argument("--split-min-work", type=int, default=None, help="hconv least taps x chunks per split")
    ap.add_argument("--bnb", action="store_true",
                    help="dgrad with the production epilogue: the consuming BatchNorm's ReLU mask (y) and "
                         "backward statistics (x, mean, istd) fused in (BnbRequest)")
    ap.add_argument("--no-group", action="store_true", help="strided dgrad phases as separate launches")
    ap.add_argument("--depthwise", action="store_true", help="depthwise kernels at the MobileNetV1-tiny shapes")
    ap.add_argument("--reps", type=int, default=5, help="--depthwise: timed replays per figure (median, min, max)")
    ap.add_argument("--torch-ref", type=int, default=1, help="--depthwise: also time PyTorch's grouped conv passes")
    ap.add_argument("--step", action="store_true", help="--depthwise: also time the captured MobileNetV1 training step")
    ap.add_argument("--json", default="", help="--depthwise: write the figures to this file as they come")
    ap.add_argument("--grouped", action="store_true",
                    help="grouped-conv kernels at the ResNeXt-50 32x4d tiny shapes (takes --reps, --torch-ref, --step, "
                         "--json like --depthwise)")
    a = ap.parse_args()
    if a.depthwise:
        return depthwise_main(a)
    if a.grouped:
        return grouped_main(a)
    from dcnn_amd.ops import hip, fusion
    if a.split_target is not None:
        hip.kernels().hconv_set_split_target(a.split_target)
    if a.split_min_work is not None:
        hip.kernels().hconv_set_split_min_work(a.split_min_work)
    hip.kernels().hconv3_enable(a.v3)
    fusion.HCONV_1X1 = bool(a.halo_1x1)
    if a.no_group:
        fusion.G2_GROUP = False
    if a.hwgrad_s2 is not None:
        fusion.HWGRAD_S2 = bool(a.hwgrad_s2)
    CL = torch.channels_last
    N = a.batch
    tot = {"fwd": 0.0, "dgrad": 0.0, "wgrad": 0.0}
    print(f"{'shape':<10}{'op':<7}{'us':>9}{'TFLOP/s':>9}{'TB/s':>7}")
    keep = set(a.shapes.split(",")) if a.shapes else None
    for (nm, Ci, H, W, Co, k, s, p) in (SHAPES_R50 if a.set == "r50" else SHAPES):
        if keep is not None and nm not in keep:
            continue
        x = torch.randn(N, Ci, H, W, device="cuda").bfloat16().contiguous(memory_format=CL)
        w = (torch.randn(Co, Ci, k, k, device="cuda") * 0.05).bfloat16().contiguous(memory_format=CL)
        wf = w
        if Ci < 8:  # the RGB stem runs channel-padded to 8 (as Conv2D does)
            x = hip.to_act_padded(x.float().contiguous(), 8)
            wf = hip.pad_weight_channels(w, 8)
        OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        dy = torch.randn(N, Co, OH, OW, device="cuda").bfloat16().contiguous(memory_format=CL)
        gw = torch.zeros(Co, Ci, k, k, device="cuda").contiguous(memory_format=CL)
        wt = hip.conv_weight_t(w)
        flops = 2.0 * N * OH * OW * Co * Ci * k * k
        # compulsory HBM bytes (bf16 operands read once, result written once; wgrad: fp32 result)
        hbm = {"fwd": 2.0 * (N * H * W * Ci + N * OH * OW * Co + Co * Ci * k * k),
               "dgrad": 2.0 * (N * H * W * Ci + N * OH * OW * Co + Co * Ci * k * k),
               "wgrad": 2.0 * (N * H * W * Ci + N * OH * OW * Co) + 4.0 * Co * Ci * k * k}
        bnb = None
        if a.bnb and Ci >= 8:
            # the BatchNorm that produced x: ReLU output y (mask), input xb, saved statistics
            from dcnn_amd.ops.hip_base import BnbRequest
            xb = torch.randn_like(x)
            bnb = BnbRequest(None, torch.relu(xb), xb, torch.zeros(Ci, device="cuda"),
                             torch.ones(Ci, device="cuda"))
            hbm["dgrad"] += 4.0 * N * H * W * Ci  # y and x read in the epilogue
        ops = {
            "fwd": lambda: hip.conv2d_fwd(x, wf, None, (s, s), (p, p), stats=True),
            "dgrad": lambda: hip.conv2d_dgrad(dy, wt, x.shape, (s, s), (p, p), bnb=bnb),
            "wgrad": lambda: hip.conv2d_wgrad(dy, x, w.shape, (s, s), (p, p), gw, None),
        }
        if a.torch_mm and k == 1 and s == 1:
            xm, dym = x.permute(0, 2, 3, 1).reshape(-1, Ci), dy.permute(0, 2, 3, 1).reshape(-1, Co)  # NHWC rows (views)
            w2 = w.reshape(Co, Ci)
            ops["mm_fwd"] = lambda: torch.mm(xm, w2.t())
            ops["mm_dgrad"] = lambda: torch.mm(dym, w2)
            ops["mm_wgrad"] = lambda: torch.mm(dym.t(), xm)
            for o in ("mm_fwd", "mm_dgrad", "mm_wgrad"):
                hbm[o] = hbm[o[3:]]
                tot.setdefault(o, 0.0)
        for op, fn in ops.items():
            if a.only and op.replace("mm_", "") != a.only:
                continue
            if op == "dgrad" and nm == "stem":
                continue
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            if a.eager:
                e0.record()
                for _ in range(a.iters):
                    fn()
                e1.record()
            else:
                # device time without host launch overhead: the calls captured into one graph
                g = torch.cuda.CUDAGraph()
                s_ = torch.cuda.Stream()
                s_.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s_):
                    with torch.cuda.graph(g, stream=s_):
                        for _ in range(a.iters):
                            fn()
                torch.cuda.current_stream().wait_stream(s_)
                g.replay()
                torch.cuda.synchronize()
                e0.record()
                g.replay()
                e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1000 / a.iters
            tot[op] += us
            print(f"{nm:<10}{op:<7}{us:9.1f}{flops / us / 1e6:9.1f}{hbm[op] / us / 1e6:7.2f}")
    print("totals (us, one pass over the shapes):", {k: round(v, 1) for k, v in tot.items()})


if __name__ == "__main__":
    main()
