#!/usr/bin/env python
"""Gradient statistics and gradient-norm clipping (szn_grad_stats, szn_clip_coef, TrainStep(clip=)) on one GPU, in one process; one
JSON line per setting.

  kernel:  szn_grad_stats over the flat weight buffer of FCN32s at E = 300 with its layer table, on the fp32 gradient and on a bf16
           image, next to szn_grad_check_finite (the same bytes) and the unchanged szn_adam_step (with its bf16 weight image) over the
           same n; each with its achieved GB/s (4, 2, 4 and 30 bytes per element) and the floor bytes / 6.29 TB/s (the measured copy
           rate); szn_clip_coef alone.
  step:    the bf16 cosine TrainStep at B = 8 and B = 1, 512 x 512, E = 300, K = 59: default, fused_adam=False, clip = inf, clip finite,
           on the same images and labels.
Per setting: warm-up, then --reps timed windows of HIP-event timing, the routes alternating window by window; median and min-max."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zeroshotsemanticsegmentation_amd import _lib as L, engine, models, synth  # noqa: E402

E, K = 300, 59
COPY_GBS = 6290.0


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def timed(routes, reps, iters, warmup):
    for _ in range(warmup):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in routes}
    for _ in range(reps):
        for k, fn in routes.items():
            ts[k].append(window(fn, iters))
    out = {}
    for k, v in ts.items():
        out[k + "_ms"] = float(np.median(v))
        out[k + "_ms_minmax"] = [float(min(v)), float(max(v))]
    return out


def bench_kernel(args, box, dev):
    m = models.FCN32s(E)
    counts = [getattr(m, n).weight.numel() for n in models.opt_layers(m)]
    n, nseg = sum(counts), len(counts)
    tab = (C.c_int64 * nseg)(*np.cumsum(counts).tolist())
    p, g, m1, m2 = (torch.randn(n, device=dev) for _ in range(4))
    m2.abs_()
    g16 = g.to(torch.bfloat16)
    lp = torch.empty(n, device=dev, dtype=torch.bfloat16)
    stats = torch.zeros(nseg, 2, dtype=torch.float64, device=dev)
    ws = torch.empty(L.load().szn_grad_stats_workspace_bytes(n, nseg), dtype=torch.uint8, device=dev)
    dyn = torch.tensor([1.0, 0.0, 0.0, 0.0], device=dev)
    clip = torch.tensor([1.0, 0.0, 0.0, 0.0], device=dev)
    st = L.stream_ptr()
    routes = {
        "stats_f32": lambda: L.call("szn_grad_stats", n, L.ptr(g), L.SZN_F32, nseg, tab, L.ptr(stats), L.ptr(ws), st),
        "stats_bf16": lambda: L.call("szn_grad_stats", n, L.ptr(g16), L.SZN_BF16, nseg, tab, L.ptr(stats), L.ptr(ws), st),
        "finite": lambda: L.call("szn_grad_check_finite", n, L.ptr(g), L.ptr(dyn), st),
        "adam": lambda: L.call("szn_adam_step", n, L.ptr(p), L.ptr(g), L.ptr(m1), L.ptr(m2), 1e-5, 0.9, 0.999, 1e-8, 0.0, 3, 1.0, L.ptr(lp),
                               L.SZN_BF16, st),
        "coef": lambda: L.call("szn_clip_coef", nseg, L.ptr(stats), 1.0, 1.0, None, L.ptr(clip), st),
    }
    res = {"box": box, "what": "kernel", "n": n, "segments": nseg}
    res.update(timed(routes, args.reps, args.kernel_iters, args.warmup))
    for k, nbytes in (("stats_f32", 4), ("stats_bf16", 2), ("finite", 4), ("adam", 30)):
        res[k + "_gbs"] = n * nbytes / res[k + "_ms"] / 1e6
        res[k + "_floor_ms"] = n * nbytes / COPY_GBS / 1e6
    res.update({"stats_f32_over_adam_gbs": res["stats_f32_gbs"] / res["adam_gbs"], "stats_bf16_over_adam_gbs": res["stats_bf16_gbs"] / res["adam_gbs"],
                "stats_f32_over_finite": res["stats_f32_ms"] / res["finite_ms"], "reps": args.reps, "iters": args.kernel_iters})
    print(json.dumps(res), flush=True)
    del p, g, m1, m2, g16, lp
    torch.cuda.empty_cache()


def bench_step(args, box, dev):
    H = args.size
    emb = synth.make_embeddings(K, E)
    for B in (args.batch, 1):
        x = torch.from_numpy(synth.make_images(B, H, H, seed=11)).to(dev)
        t = torch.from_numpy(synth.make_labels(B, H, H, K, seed=12, block=16)).to(dev)
        steps = {}
        for name, kw in (("default", {}), ("unfused", dict(fused_adam=False)), ("clip_inf", dict(clip=dict(max_norm=float("inf")))),
                         ("clip", dict(clip=dict(max_norm=args.max_norm)))):
            m = models.FCN32s(E).load_synthetic(1337, device=dev).train()
            steps[name] = engine.TrainStep(m, emb, loss="cos", optimizer="adam", lr=1e-5, precision=torch.bfloat16, keep_grads=False, **kw)
        res = {"box": box, "what": "step", "loss": "cos", "B": B, "H": H, "W": H, "E": E, "K": K, "precision": "bf16", "max_norm": args.max_norm}
        iters = args.step_iters if B > 1 else 4 * args.step_iters
        res.update(timed({k + "_step": (lambda s=s: s.step(x, t)) for k, s in steps.items()}, args.reps, iters, args.warmup + 1))
        r = steps["clip"].grad_norms()
        res.update({"unfused_extra_ms": res["unfused_step_ms"] - res["default_step_ms"],
                    "clip_inf_over_unfused_ms": res["clip_inf_step_ms"] - res["unfused_step_ms"],
                    "clip_over_unfused_ms": res["clip_step_ms"] - res["unfused_step_ms"],
                    "clip_over_default": res["clip_step_ms"] / res["default_step_ms"],
                    "clipped_steps": r["clipped"], "steps_seen": r["seen"], "last_norm": r["norm"], "reps": args.reps, "iters": iters})
        print(json.dumps(res), flush=True)
        del steps
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--kernel-iters", type=int, default=20)
    ap.add_argument("--step-iters", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--max-norm", type=float, default=1e-3, help="the finite max_norm of the `clip` step configuration")
    ap.add_argument("--only", choices=["kernel", "step"], default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_clip: needs a GPU")
    L.load()
    dev = torch.device("cuda", 0)
    box = torch.cuda.get_device_name(0)
    if args.only != "step":
        bench_kernel(args, box, dev)
    if args.only != "kernel":
        bench_step(args, box, dev)


if __name__ == "__main__":
    main()
