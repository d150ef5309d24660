#!/usr/bin/env python
"""Gradient accumulation (szn_grad_accum, TrainStep(accum=)) on one GPU, in one process; one JSON line per setting (DESIGN.md section
7w).

  kernel:  szn_grad_accum SET, ADD and FINAL over the flat weight buffer of FCN32s at E = 300 (8, 12 and 12 bytes per element) next to
           szn_ema_step (the same three streams as ADD / FINAL), the unchanged szn_adam_step (with its bf16 weight image, 30 bytes) and
           torch's copy_ (SET's two streams) over the same n; each with its achieved GB/s.
  step:    the bf16 cosine TrainStep at B = 8 and B = 1, 512 x 512, E = 300, K = 59: default, fused_adam=False, and accum steps = A
           (default 4), whose non-boundary and boundary calls are timed separately (one HIP event per call inside whole windows); the
           per-image cost of a window against A default steps.
Per setting: warm-up, then --reps timed windows of HIP-event timing, the routes alternating window by window; median and min-max."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zeroshotsemanticsegmentation_amd import _lib as L, engine, models, synth  # noqa: E402

E, K = 300, 59


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def summary(ts):
    out = {}
    for k, v in ts.items():
        out[k + "_ms"] = float(np.median(v))
        out[k + "_ms_minmax"] = [float(min(v)), float(max(v))]
    return out


def timed(routes, reps, iters, warmup):
    for _ in range(warmup):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in routes}
    for _ in range(reps):
        for k, fn in routes.items():
            ts[k].append(window(fn, iters))
    return summary(ts)


def bench_kernel(args, box, dev):
    m = models.FCN32s(E)
    n = sum(getattr(m, name).weight.numel() for name in models.opt_layers(m))
    p, g, g2, m1, m2, acc, avg = (torch.randn(n, device=dev) for _ in range(7))
    m2.abs_()
    lp = torch.empty(n, device=dev, dtype=torch.bfloat16)
    st = L.stream_ptr()
    routes = {
        "set": lambda: L.call("szn_grad_accum", n, L.ptr(acc), L.ptr(g), L.ACCUM_SET, st),
        "add": lambda: L.call("szn_grad_accum", n, L.ptr(acc), L.ptr(g), L.ACCUM_ADD, st),
        "final": lambda: L.call("szn_grad_accum", n, L.ptr(acc), L.ptr(g), L.ACCUM_FINAL, st),
        "ema": lambda: L.call("szn_ema_step", n, L.ptr(avg), L.ptr(p), 0.999, 1, 0, None, st),
        "adam": lambda: L.call("szn_adam_step", n, L.ptr(p), L.ptr(g2), L.ptr(m1), L.ptr(m2), 1e-5, 0.9, 0.999, 1e-8, 0.0, 3, 1.0, L.ptr(lp),
                               L.SZN_BF16, st),
        "copy": lambda: avg.copy_(p),
    }
    # (adam reads a gradient buffer of its own: g grows under FINAL)
    res = {"box": box, "what": "kernel", "n": n}
    res.update(timed(routes, args.reps, args.kernel_iters, args.warmup))
    for k, nbytes in (("set", 8), ("add", 12), ("final", 12), ("ema", 12), ("adam", 30), ("copy", 8)):
        res[k + "_gbs"] = n * nbytes / res[k + "_ms"] / 1e6
    res.update({"add_over_ema": res["add_ms"] / res["ema_ms"], "final_over_ema": res["final_ms"] / res["ema_ms"],
                "set_over_add": res["set_ms"] / res["add_ms"], "set_over_copy": res["set_ms"] / res["copy_ms"],
                "ema_spread": (res["ema_ms_minmax"][1] - res["ema_ms_minmax"][0]) / res["ema_ms"],
                "reps": args.reps, "iters": args.kernel_iters})
    print(json.dumps(res), flush=True)
    del p, g, g2, m1, m2, acc, avg, lp
    torch.cuda.empty_cache()


def windows_per_call(ts, x, t, A, reps, windows):
    """whole windows of A calls with one event per call -> {"micro": [ms per non-boundary call], "boundary": [...], "window": [...]},
    one entry per rep (the mean over the rep's windows)"""
    out = {"micro": [], "boundary": [], "window": []}
    for _ in range(reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(windows * A + 1)]
        torch.cuda.synchronize()
        ev[0].record()
        for i in range(windows * A):
            ts.step(x, t)
            ev[i + 1].record()
        torch.cuda.synchronize()
        dt = [ev[i].elapsed_time(ev[i + 1]) for i in range(windows * A)]
        out["micro"].append(float(np.mean([d for i, d in enumerate(dt) if (i + 1) % A])))
        out["boundary"].append(float(np.mean([d for i, d in enumerate(dt) if not (i + 1) % A])))
        out["window"].append(ev[0].elapsed_time(ev[-1]) / windows)
    return out


def bench_step(args, box, dev):
    H, A = args.size, args.accum
    emb = synth.make_embeddings(K, E)
    for B in (args.batch, 1):
        x = torch.from_numpy(synth.make_images(B, H, H, seed=11)).to(dev)
        t = torch.from_numpy(synth.make_labels(B, H, H, K, seed=12, block=16)).to(dev)
        steps = {}
        for name, kw in (("default", {}), ("unfused", dict(fused_adam=False)), ("accum", dict(accum=dict(steps=A)))):
            m = models.FCN32s(E).load_synthetic(1337, device=dev).train()
            steps[name] = engine.TrainStep(m, emb, loss="cos", optimizer="adam", lr=1e-5, precision=torch.bfloat16, keep_grads=False, **kw)
        res = {"box": box, "what": "step", "loss": "cos", "B": B, "H": H, "W": H, "E": E, "K": K, "precision": "bf16", "accum_steps": A}
        iters = args.step_iters if B > 1 else 4 * args.step_iters
        windows = max(1, iters // A)
        for _ in range(args.warmup + 1):
            for s in steps.values():
                for _ in range(A):
                    s.step(x, t)
        ts = {"default_step": [], "unfused_step": [], "accum_micro": [], "accum_boundary": [], "accum_window": []}
        for _ in range(args.reps):                                           # the routes alternate rep by rep
            ts["default_step"].append(window(lambda: steps["default"].step(x, t), windows * A))
            ts["unfused_step"].append(window(lambda: steps["unfused"].step(x, t), windows * A))
            w = windows_per_call(steps["accum"], x, t, A, 1, windows)
            for k in ("micro", "boundary", "window"):
                ts["accum_" + k].append(w[k][0])
        res.update(summary(ts))
        per_image_accum = res["accum_window_ms"] / (A * B)
        per_image_default = res["default_step_ms"] / B
        res.update({"unfused_extra_ms": res["unfused_step_ms"] - res["default_step_ms"],
                    "micro_over_default_ms": res["accum_micro_ms"] - res["default_step_ms"],
                    "boundary_over_unfused_ms": res["accum_boundary_ms"] - res["unfused_step_ms"],
                    "per_image_accum_ms": per_image_accum, "per_image_default_ms": per_image_default,
                    "per_image_accum_over_default": per_image_accum / per_image_default,
                    "applied_steps": steps["accum"].applied_steps, "reps": args.reps, "calls_per_rep": windows * A})
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
    ap.add_argument("--accum", type=int, default=4, help="the window length A of the accumulating step")
    ap.add_argument("--only", choices=["kernel", "step"], default=None)
    args = ap.parse_args()
    if args.accum < 2:
        raise SystemExit("bench_accum: --accum must be at least 2")
    if not torch.cuda.is_available():
        raise SystemExit("bench_accum: needs a GPU")
    L.load()
    dev = torch.device("cuda", 0)
    box = torch.cuda.get_device_name(0)
    if args.only != "step":
        bench_kernel(args, box, dev)
    if args.only != "kernel":
        bench_step(args, box, dev)


if __name__ == "__main__":
    main()
