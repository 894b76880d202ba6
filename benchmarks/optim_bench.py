#!/usr/bin/env python3
"""Optimizer-step micro-benchmark: the gradient-norm reduction, the plain fused Adam step, the tail
kernel with clip only / EMA only / both, the weight <-> EMA exchange, and the layer-wise LAMB and LARS steps
(two launches each, over the model's own segment / chunk tables) next to the plain Adam and SGD steps, at
the parameter arenas of ``resnet18_tiny_imagenet`` and ``convnext_tiny_tiny_imagenet``
(profiles/clip_ema.md, profiles/lamb_lars.md).

Every kernel is timed against a device copy that moves the same number of bytes, the rows alternating
round after round in one process. A window is ``--iters`` (>= 200) launches captured in a hipGraph and
replayed between two device events after a warm-up (no Python launch cost inside the window); the
figure is the median of ``--rounds`` windows. Bytes per parameter come from the design, not from a
counter: the plain Adam step reads p, g, m, v and writes p, m, v and the bf16 shadow, 4 * 4 + 3 * 4 + 2 =
30 B; the clip adds the 4 B read of the reduction (the coefficient itself is one float); the EMA adds its
read and write, 8 B; the exchange reads and writes both buffers and writes the shadow, 18 B. LAMB reads p, g,
m, v and writes m, v (24 B), then reads p, m, v and writes p and the shadow (18 B): 42 B; LARS with momentum
reads p, g (8 B), then reads p, g, v and writes p, v and the shadow (22 B): 30 B against the SGD step's 22 B.
The two passes of a layer-wise step are separate kernels: their individual times come from a kernel trace of
this script (``--only layerwise`` keeps the traced run short), not from these windows.

  python benchmarks/optim_bench.py [--md optim_bench.md]
  python benchmarks/optim_bench.py --step [--batch 256]     # the ResNet-18 captured step, switches on / off
  python benchmarks/optim_bench.py --step --step-opt lamb   # ... the same step with LAMB against Adam
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODELS = ["resnet18_tiny_imagenet", "convnext_tiny_tiny_imagenet"]
HP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, bc1=0.19, bc2=0.002, wd=0.05, decoupled=True)


def arena_of(name):
    from dcnn_amd.models import create_model
    m = create_model(name)
    m.set_seed(0)
    m.initialize()
    return m.arena


def arena_size(name):
    return arena_of(name).numel


def kernels_table(a):
    from dcnn_amd.ops import hip
    dev = torch.device("cuda")
    # one capture stream, its ticket word of the reduction created before any capture (created
    # inside one, its zeroing would be replayed)
    cs = torch.cuda.Stream()
    with torch.cuda.stream(cs):
        hip.prewarm_tickets(dev, ("gradnorm", "layerwise"))
    torch.cuda.synchronize()

    def window(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=cs):
            for _ in range(a.iters):
                fn()
        gr.replay()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def run():
            e0.record()
            for _ in range(a.replays):
                gr.replay()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / (a.iters * a.replays)  # us per launch
        return run

    rows = []
    for name in MODELS:
        from dcnn_amd.nn.params import SegmentTables
        host = arena_of(name)
        n = host.numel
        counts = [int(torch.tensor(sp.shape).prod()) for sp in host.specs]
        tables = SegmentTables.from_slices(host.offsets, counts, host.no_decay_flags(), True, n, dev)
        ws = hip.layerwise_workspace(tables, dev)
        g = torch.Generator().manual_seed(0)
        p, grad, ema = (torch.randn(n, generator=g).to(dev) for _ in range(3))
        m = torch.zeros(n, device=dev)
        v = torch.zeros(n, device=dev)
        shadow = torch.zeros(n, dtype=torch.bfloat16, device=dev)
        blk = torch.tensor([0.0, 0.0, 0.999, 1.0], device=dev)
        hyper = torch.tensor([HP["lr"], HP["bc1"], HP["bc2"], 1.0], device=dev)
        args = (p, grad, m, v, shadow, HP["lr"], HP["b1"], HP["b2"], HP["eps"], HP["bc1"], HP["bc2"], HP["wd"],
                HP["decoupled"], hyper)

        def both():
            hip.grad_sumsq(grad, 1.0, blk)
            hip.adam_step_tail(*args, coef=blk[2:3], ema=ema, ema_decay=0.9999)

        def clip():
            hip.grad_sumsq(grad, 1.0, blk)
            hip.adam_step_tail(*args, coef=blk[2:3])

        cases = [
            ("grad_sumsq", 4, lambda: hip.grad_sumsq(grad, 1.0, blk)),
            ("adam_step (plain)", 30, lambda: hip.adam_step(*args)),
            ("adam_tail, clip coefficient only", 30, lambda: hip.adam_step_tail(*args, coef=blk[2:3])),
            ("grad_sumsq + adam_tail (clip)", 34, clip),
            ("adam_tail, EMA only", 38, lambda: hip.adam_step_tail(*args, ema=ema, ema_decay=0.9999)),
            ("grad_sumsq + adam_tail (clip + EMA)", 42, both),
            ("ema_swap", 18, lambda: hip.ema_swap(p, ema, shadow)),
            ("sgd_step (plain, momentum)", 22, lambda: hip.sgd_step(p, grad, m, shadow, HP["lr"], 0.9, hyper)),
            ("lamb_step (moments + apply)", 42,
             lambda: hip.lamb_step(p, grad, m, v, shadow, HP["lr"], HP["b1"], HP["b2"], 1e-6, HP["bc1"], HP["bc2"],
                                   HP["wd"], tables, *ws, hyper=hyper)),
            ("lars_step (norms + apply, momentum)", 30,
             lambda: hip.lars_step(p, grad, m, shadow, HP["lr"], 0.9, 5e-4, 1e-3, 1e-8, tables, *ws, hyper=hyper)),
        ]
        if a.only == "layerwise":
            cases = [c for c in cases if c[0].startswith(("adam_step (plain)", "sgd_step", "lamb_step", "lars_step"))]
        runs = []
        for label, bpp, fn in cases:
            nbytes = bpp * n
            src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            runs.append((label, bpp, window(fn), window(lambda: dst.copy_(src)), src, dst))  # (keeps the buffers alive)
        times = {label: ([], []) for label, *_ in runs}
        for _ in range(a.rounds):  # alternating: every row's kernel and its copy, round after round
            for label, _, rk, rc, *_ in runs:
                times[label][0].append(rk())
                times[label][1].append(rc())
        for label, bpp, *_ in runs:
            tk, tc = statistics.median(times[label][0]), statistics.median(times[label][1])
            rows.append(dict(model=name, n=n, kernel=label, bytes_per_param=bpp, us=round(tk, 2),
                             gbps=round(bpp * n / tk / 1e3, 1), copy_us=round(tc, 2),
                             copy_gbps=round(bpp * n / tc / 1e3, 1), fraction_of_copy=round(tc / tk, 3)))
            print(json.dumps(rows[-1]), flush=True)
        del p, grad, ema, m, v, shadow
        torch.cuda.empty_cache()
    return rows


def step_table(a):
    """ResNet-18 b256, the Python engine's captured step (bench.py's workload), max_grad_norm 1.0 and
    ema_decay 0.9999 (or, with --step-opt, LAMB / LARS) against the plain Adam step: two steps in one
    process, alternating rounds."""
    from dcnn_amd.models import INPUT_SHAPES, NUM_CLASSES, create_model
    from dcnn_amd.nn import Adam, LossFactory
    from dcnn_amd.runtime.step import TrainStep
    name = "resnet18_tiny_imagenet"
    dev = torch.device("cuda")
    C, H, W = INPUT_SHAPES[name]
    g = torch.Generator().manual_seed(0)
    x = torch.randn(a.batch, C, H, W, generator=g).to(dev)
    y = torch.randint(0, NUM_CLASSES[name], (a.batch,), generator=g).to(dev)
    steps = {}
    from dcnn_amd.nn import LAMB, LARS
    make = {"tail": lambda: Adam(1e-3, max_grad_norm=1.0, ema_decay=0.9999), "lamb": lambda: LAMB(1e-3),
            "lars": lambda: LARS(0.1)}[a.step_opt]
    for label, ctor in (("off", lambda: Adam(1e-3)), ("on", make)):
        m = create_model(name)
        m.set_seed(1234)
        m.set_device("GPU:0")
        m.initialize()
        m.set_first_layer_input_grad(False)
        opt = ctor()
        opt.attach(m)
        st = TrainStep(m, LossFactory.create("softmax_crossentropy"), opt, use_graph=True)
        for _ in range(5):
            st(x, y)
        torch.cuda.synchronize()
        steps[label] = st
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {"off": [], "on": []}
    for _ in range(a.rounds):
        for label in ("off", "on"):
            e0.record()
            for _ in range(a.steps):
                steps[label](x, y)
            e1.record()
            e1.synchronize()
            times[label].append(e0.elapsed_time(e1) / a.steps)
    off, on = statistics.median(times["off"]), statistics.median(times["on"])
    rec = dict(model=name, batch=a.batch, on=a.step_opt, step_ms_off=round(off, 4), step_ms_on=round(on, 4),
               cost_percent=round((on / off - 1) * 100, 2), rounds_off=[round(t, 4) for t in times["off"]],
               rounds_on=[round(t, 4) for t in times["on"]])
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200, help="launches per captured window (>= 200)")
    ap.add_argument("--replays", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--md", default=None, help="also write the markdown table to this file")
    ap.add_argument("--step", action="store_true", help="the captured ResNet-18 step, switches on against off")
    ap.add_argument("--step-opt", choices=["tail", "lamb", "lars"], default="tail",
                    help="--step: what runs against the plain Adam step: Adam with clip + EMA, LAMB or LARS")
    ap.add_argument("--only", choices=["layerwise"], default=None,
                    help="the kernel table's plain Adam / SGD and LAMB / LARS rows alone")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=30, help="--step: training steps per window")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench: needs a GPU (nothing is measured without one)")
    if a.iters < 200:
        raise SystemExit("optim_bench: a window is at least 200 launches")
    if a.step:
        rec = step_table(a)
        on = {"tail": "both on", "lamb": "LAMB", "lars": "LARS"}[a.step_opt]
        lines = [f"| model | batch | step, plain Adam (ms) | step, {on} (ms) | cost |", "|---|---|---|---|---|",
                 f"| {rec['model']} | {rec['batch']} | {rec['step_ms_off']} | {rec['step_ms_on']} | "
                 f"{rec['cost_percent']} % |"]
    else:
        rows = kernels_table(a)
        lines = ["| arena | kernel | B / param | us | GB/s | same-bytes copy us | copy GB/s | fraction of the copy |",
                 "|---|---|---|---|---|---|---|---|"]
        for r in rows:
            lines.append(f"| {r['model']} ({r['n']}) | {r['kernel']} | {r['bytes_per_param']} | {r['us']} | {r['gbps']} | "
                         f"{r['copy_us']} | {r['copy_gbps']} | {r['fraction_of_copy']} |")
    print("\n".join(lines))
    if a.md:
        os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
        with open(a.md, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
