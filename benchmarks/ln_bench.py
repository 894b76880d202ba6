#!/usr/bin/env python3
"""Channel LayerNorm / LayerScale / GELU micro-benchmark at the ConvNeXt-T activation shapes
(bf16 NHWC rows, batch 128: R x C = 32768 x 96, 8192 x 192, 2048 x 384, 512 x 768, GELU on the 4C
tensors).

Every op is timed against two yardsticks in the same process, the three alternating round after
round: a device copy that moves the same number of bytes, and PyTorch-ROCm's op on the same data
(F.layer_norm / native_layer_norm_backward, F.gelu / gelu_backward, an elementwise expression for
LayerScale). A window is `--iters` calls captured in a hipGraph and replayed `--replays` times
between two device events (no Python launch cost inside the window); the figure is the median of
`--rounds` windows. Bytes are what the algorithm must move (the activation tensors; the per-channel
vectors and per-row statistics are negligible), computed from the shapes here.

These tensors (0.8 - 19 MB) fit the last-level cache: the rates are cache rates, the same for the
copy, which is why the copy and not an HBM peak is the yardstick.

  python benchmarks/ln_bench.py [--batch 128] [--md ln_bench.md]

``--drop-path`` measures stochastic depth instead (profiles/drop_path.md): at the ConvNeXt-pico and
ConvNeXt-T block shapes, the fused drop tail (lscale_drop_fwd / lscale_drop_bwd, mask drawn at
``--rate``) against the unmasked scale tail (lscale_fwd with residual / lscale_bwd) and against the
unfused composition (LayerScale, standalone DropPath, add), the three alternating round after round;
then a ConvNeXt-pico training step (captured) at drop-path rates 0 and ``--rate``, alternating.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# ConvNeXt-T on 64x64 inputs: (stage, C, map side)
STAGES = [("s1", 96, 16), ("s2", 192, 8), ("s3", 384, 4), ("s4", 768, 2)]
EPS = 1e-6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--md", default=None, help="also write the markdown table to this file")
    ap.add_argument("--drop-path", action="store_true", help="the stochastic-depth rows instead")
    ap.add_argument("--rate", type=float, default=0.1, help="--drop-path: the drop rate of the mask")
    ap.add_argument("--steps", type=int, default=30, help="--drop-path: training steps per window")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ln_bench: needs a GPU (nothing is measured without one)")
    from dcnn_amd.nn.activations import ActivationFactory
    from dcnn_amd.ops import hip
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    gelu = ActivationFactory.create("gelu")
    aten = torch.ops.aten

    def window(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for _ in range(a.iters):
                fn()
        gr.replay()
        torch.cuda.synchronize()

        def run():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.replays):
                gr.replay()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / (a.replays * a.iters)  # us per call
        return run

    if a.drop_path:
        return drop_path_rows(a, window)

    rows = []
    lines = ["| shape R x C | op | tensors | MB | ours us | ours TB/s | copy us | % of copy | torch us | torch / ours |",
             "|---|---|---:|---:|---:|---:|---:|---:|---:|---:|"]
    print("\n".join(lines), flush=True)
    for nm, C, side in STAGES:
        R = a.batch * side * side
        mk = lambda c: torch.randn(R, c, generator=g).to(dev).to(torch.bfloat16)  # noqa: E731
        x, dy, res = mk(C), mk(C), mk(C)
        xw, dyw = mk(4 * C), mk(4 * C)
        gamma = (1 + 0.1 * torch.randn(C, generator=g)).to(dev)
        beta = (0.1 * torch.randn(C, generator=g)).to(dev)
        gb, bb = gamma.bfloat16(), beta.bfloat16()
        _, mean, rstd = hip.ln_fwd(x, gamma, beta, EPS)
        _, tmean, trstd = aten.native_layer_norm(x, [C], gb, bb, EPS)
        dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        yw = gelu.apply(xw)
        ops = [
            ("ln_fwd", x, 2, lambda: hip.ln_fwd(x, gamma, beta, EPS), lambda: F.layer_norm(x, (C,), gb, bb, EPS)),
            ("ln_bwd", x, 3, lambda: hip.ln_bwd(dy, x, gamma, mean, rstd, dg, db),
             lambda: aten.native_layer_norm_backward(dy, x, [C], tmean, trstd, gb, bb, [True, True, True])),
            # dx only (no affine): the main pass without the slab write and the slab reduce launch
            ("ln_bwd dx only", x, 3, lambda: hip.ln_bwd(dy, x, None, mean, rstd, None, None),
             lambda: aten.native_layer_norm_backward(dy, x, [C], tmean, trstd, None, None, [True, False, False])),
            ("lscale_fwd+res", x, 3, lambda: hip.lscale_fwd(x, gamma, res), lambda: torch.addcmul(res, x, gb)),
            ("lscale_bwd", x, 3, lambda: hip.lscale_bwd(dy, x, gamma, dg),
             lambda: (dy * gb, (dy.float() * x.float()).sum(0))),
            ("gelu_fwd (4C)", xw, 2, lambda: gelu.apply(xw), lambda: F.gelu(xw)),
            ("gelu_bwd (4C)", xw, 3, lambda: gelu.gradient(xw, yw, dyw), lambda: aten.gelu_backward(dyw, xw)),
        ]
        for op, t, nt, ours, theirs in ops:
            nbytes = nt * t.numel() * 2
            src = torch.empty(nbytes // 4, dtype=torch.bfloat16, device=dev).normal_()  # copy: read + write = nbytes
            dst = torch.empty_like(src)
            wins = [window(ours), window(lambda: dst.copy_(src)), window(theirs)]
            ts = [[], [], []]
            for _ in range(a.rounds):  # alternate the three
                for k, w in enumerate(wins):
                    ts[k].append(w())
            us, cp, th = (statistics.median(v) for v in ts)
            mb = nbytes / 1e6
            r = dict(shape=f"{R}x{t.shape[1]}", op=op, tensors=nt, MB=round(mb, 2), ours_us=round(us, 2),
                     ours_tbps=round(mb / us, 2), copy_us=round(cp, 2), pct_of_copy=round(100 * cp / us, 1),
                     torch_us=round(th, 2), torch_over_ours=round(th / us, 2),
                     spread_us=[round(min(ts[0]), 2), round(max(ts[0]), 2)])
            rows.append(r)
            lines.append(f"| {R} x {t.shape[1]} | {op} | {nt} | {mb:.2f} | {us:.2f} | {mb / us:.2f} | {cp:.2f} | "
                         f"{100 * cp / us:.0f}% | {th:.2f} | {th / us:.2f} |")
            print(lines[-1], flush=True)
    for r in rows:
        print(json.dumps(r))
    if a.md:
        with open(a.md, "w") as f:
            f.write("\n".join(lines) + "\n")


def drop_path_rows(a, window):
    from dcnn_amd.ops import hip
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    N = a.batch
    # (model, C, map side): ConvNeXt-pico on 32x32 inputs, ConvNeXt-T on 64x64
    shapes = [("pico", 64, 16), ("pico", 128, 8), ("pico", 256, 4), ("pico", 512, 2),
              ("T", 96, 16), ("T", 192, 8), ("T", 384, 4), ("T", 768, 2)]
    lines = ["| model | N x C x H x W | pass | drop tail us | scale tail us | unfused us | drop / scale | drop / unfused "
             "| spread drop us | spread scale us |", "|---|---|---|---:|---:|---:|---:|---:|---|---|"]
    print("\n".join(lines), flush=True)
    rows = []
    for model, C, side in shapes:
        mk = lambda: torch.randn(N, C, side, side, generator=g).to(dev).to(torch.bfloat16).contiguous(  # noqa: E731
            memory_format=torch.channels_last)
        x, dy, res = mk(), mk(), mk()
        gamma = (1 + 0.1 * torch.randn(C, generator=g)).to(dev)
        dg = torch.zeros(C, device=dev)
        mask = hip.drop_path_mask(torch.zeros(N, device=dev), a.rate, 1234, draw=1)
        passes = [
            ("fwd", lambda: hip.lscale_drop_fwd(x, gamma, mask, res), lambda: hip.lscale_fwd(x, gamma, res),
             lambda: hip.drop_path_scale(hip.lscale_fwd(x, gamma), mask) + res),
            ("bwd", lambda: hip.lscale_drop_bwd(dy, x, gamma, mask, dg), lambda: hip.lscale_bwd(dy, x, gamma, dg),
             lambda: hip.lscale_bwd(hip.drop_path_scale(dy, mask), x, gamma, dg)),
        ]
        for nm, fused, plain, unfused in passes:
            wins = [window(fused), window(plain), window(unfused)]
            ts = [[], [], []]
            for _ in range(a.rounds):  # alternate the three
                for k, w in enumerate(wins):
                    ts[k].append(w())
            f, p, u = (statistics.median(v) for v in ts)
            r = dict(model=model, shape=[N, C, side, side], op=nm, rate=a.rate, kept=int((mask != 0).sum()),
                     drop_tail_us=round(f, 2), scale_tail_us=round(p, 2), unfused_us=round(u, 2),
                     spread_drop_us=[round(min(ts[0]), 2), round(max(ts[0]), 2)],
                     spread_scale_us=[round(min(ts[1]), 2), round(max(ts[1]), 2)],
                     spread_unfused_us=[round(min(ts[2]), 2), round(max(ts[2]), 2)])
            rows.append(r)
            lines.append(f"| {model} | {N} x {C} x {side} x {side} | {nm} | {f:.2f} | {p:.2f} | {u:.2f} | {f / p:.2f} | "
                         f"{f / u:.2f} | {min(ts[0]):.2f} - {max(ts[0]):.2f} | {min(ts[1]):.2f} - {max(ts[1]):.2f} |")
            print(lines[-1], flush=True)
    # a ConvNeXt-pico training step (captured whole) at rates 0 and --rate, alternating windows
    from dcnn_amd.models import create_model
    from dcnn_amd.nn import AdamW, LossFactory
    from dcnn_amd.runtime.step import TrainStep
    xb = torch.randn(N, 3, 32, 32, generator=g).to(dev)
    yb = torch.randint(0, 10, (N,), generator=g).to(dev)
    steps = {}
    for rate in (0.0, a.rate):
        m = create_model("convnext_pico_cifar10", drop_path_rate=rate)
        m.set_seed(1)
        m.set_device("GPU:0")
        m.initialize()
        m.set_first_layer_input_grad(False)
        opt = AdamW(1e-3, weight_decay=0.05)
        opt.attach(m)
        st = TrainStep(m, LossFactory.create("softmax_crossentropy"), opt, use_graph=True)
        for _ in range(3):
            st(xb, yb)
        torch.cuda.synchronize()
        steps[rate] = st
    ts = {r: [] for r in steps}
    for _ in range(a.rounds):
        for rate, st in steps.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                st(xb, yb)
            e1.record()
            torch.cuda.synchronize()
            ts[rate].append(e0.elapsed_time(e1) / a.steps)  # ms per step
    lines += ["", "| ConvNeXt-pico step, batch | drop-path rate | ms / step (median) | spread ms | img/s |", "|---|---:|---:|---|---:|"]
    for rate, v in ts.items():
        med = statistics.median(v)
        rows.append(dict(model="pico step", batch=N, rate=rate, ms_per_step=round(med, 3),
                         spread_ms=[round(min(v), 3), round(max(v), 3)], img_per_s=round(N / med * 1e3, 1)))
        lines.append(f"| {N} | {rate} | {med:.3f} | {min(v):.3f} - {max(v):.3f} | {N / med * 1e3:.0f} |")
        print(lines[-1], flush=True)
    for r in rows:
        print(json.dumps(r))
    if a.md:
        with open(a.md, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
