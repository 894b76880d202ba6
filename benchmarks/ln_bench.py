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


if __name__ == "__main__":
    main()
