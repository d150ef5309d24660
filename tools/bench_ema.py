#!/usr/bin/env python
"""Averaged weights (szn_ema_step, szn_swap_f32, TrainStep(ema=)) on one GPU, in one process; one JSON line per setting (DESIGN.md
section 7u).

  kernel:  szn_ema_step over the flat weight buffer of FCN32s at E = 300 next to szn_adam_step (with its bf16 weight image) and
           szn_swap_f32 over the same n, each with its achieved GB/s (12, 30 and 16 bytes per element) and share of 8 TB/s; with
           --capped-lib also the two new kernels of a second build whose grid is capped at 2048 blocks
           (make EXTRA=-DSZN_EMA_MAX_BLOCKS=2048 BUILD=build_exp LIB=../lib_exp/libszn_hip.so).
  step:    the bf16 cosine TrainStep at B = 8 and B = 1, 512 x 512, E = 300, K = 59: plain, ema every step, ema every 4th step, on the
           same images and labels.
  swap:    one averaged_weights() entry plus exit on that step (two exchanges and two casts of the 16-bit image each way).
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
PEAK_GBS = 8000.0


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


def flat_weight_count(dev):
    m = models.FCN32s(E)
    return sum(getattr(m, n).weight.numel() for n in models.opt_layers(m))


def bench_kernel(args, box, dev):
    n = flat_weight_count(dev)
    p, g, m1, m2, avg, other = (torch.randn(n, device=dev) for _ in range(6))
    m2.abs_()
    lp = torch.empty(n, device=dev, dtype=torch.bfloat16)
    st = L.stream_ptr()
    routes = {
        "ema": lambda: L.call("szn_ema_step", n, L.ptr(avg), L.ptr(p), 0.999, 1, 0, None, st),
        "adam": lambda: L.call("szn_adam_step", n, L.ptr(p), L.ptr(g), L.ptr(m1), L.ptr(m2), 1e-5, 0.9, 0.999, 1e-8, 0.0, 3, 1.0, L.ptr(lp),
                               L.SZN_BF16, st),
        "swap": lambda: L.call("szn_swap_f32", n, L.ptr(avg), L.ptr(other), st),
    }
    if args.capped_lib:             # the same two entry points of a second build (grid capped at 2048 blocks), same buffers, same process
        capped = C.CDLL(args.capped_lib)
        for name in ("szn_ema_step", "szn_swap_f32"):
            getattr(capped, name).restype, getattr(capped, name).argtypes = L.SIGNATURES[name]

        def ema_capped():
            assert capped.szn_ema_step(n, L.ptr(avg), L.ptr(p), 0.999, 1, 0, None, st) == 0

        def swap_capped():
            assert capped.szn_swap_f32(n, L.ptr(avg), L.ptr(other), st) == 0
        routes.update({"ema_capped": ema_capped, "swap_capped": swap_capped})
    res = {"box": box, "what": "kernel", "n": n}
    res.update(timed(routes, args.reps, args.kernel_iters, args.warmup))
    if args.capped_lib:
        res.update({"capped_over_ema": res["ema_capped_ms"] / res["ema_ms"], "capped_over_swap": res["swap_capped_ms"] / res["swap_ms"]})
    for k, nbytes in (("ema", 12), ("adam", 30), ("swap", 16)):
        res[k + "_gbs"] = n * nbytes / res[k + "_ms"] / 1e6
        res[k + "_share_of_8tbs"] = res[k + "_gbs"] / PEAK_GBS
    res.update({"ema_over_adam": res["ema_ms"] / res["adam_ms"], "reps": args.reps, "iters": args.kernel_iters})
    print(json.dumps(res), flush=True)
    del p, g, m1, m2, avg, other, lp
    torch.cuda.empty_cache()


def bench_step(args, box, dev):
    H = args.size
    emb = synth.make_embeddings(K, E)
    for B in (args.batch, 1):
        x = torch.from_numpy(synth.make_images(B, H, H, seed=11)).to(dev)
        t = torch.from_numpy(synth.make_labels(B, H, H, K, seed=12, block=16)).to(dev)
        steps = {}
        for name, ema in (("plain", None), ("ema1", dict(decay=0.999, every=1)), ("ema4", dict(decay=0.999, every=4))):
            m = models.FCN32s(E).load_synthetic(1337, device=dev).train()
            steps[name] = engine.TrainStep(m, emb, loss="cos", optimizer="adam", lr=1e-5, precision=torch.bfloat16, keep_grads=False,
                                           ema=ema)
        res = {"box": box, "what": "step", "loss": "cos", "B": B, "H": H, "W": H, "E": E, "K": K, "precision": "bf16"}
        iters = args.step_iters if B > 1 else 4 * args.step_iters        # (a multiple of 4: every window holds the same share of updates)
        res.update(timed({k + "_step": (lambda s=s: s.step(x, t)) for k, s in steps.items()}, args.reps, iters, args.warmup + 1))
        res.update({"ema1_extra_ms": res["ema1_step_ms"] - res["plain_step_ms"], "ema4_extra_ms": res["ema4_step_ms"] - res["plain_step_ms"],
                    "ema1_over_plain": res["ema1_step_ms"] / res["plain_step_ms"], "ema4_over_plain": res["ema4_step_ms"] / res["plain_step_ms"],
                    "ema1_updates": steps["ema1"].ema_updates, "ema4_updates": steps["ema4"].ema_updates, "reps": args.reps, "iters": iters})
        print(json.dumps(res), flush=True)
        if B > 1:
            ts = steps["ema1"]

            def visit():
                with ts.averaged_weights():
                    pass
            sw = {"box": box, "what": "swap", "n_w": ts.flat_w.numel(), "n_b": ts.flat_b.numel(), "precision": "bf16"}
            sw.update(timed({"enter_exit": visit}, args.reps, args.kernel_iters, args.warmup))
            sw.update({"reps": args.reps, "iters": args.kernel_iters})
            print(json.dumps(sw), flush=True)
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
    ap.add_argument("--only", choices=["kernel", "step"], default=None)
    ap.add_argument("--capped-lib", default=None, help="a build of the library with -DSZN_EMA_MAX_BLOCKS=2048: its two kernels are timed "
                                                       "next to this build's")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ema: needs a GPU")
    L.load()
    dev = torch.device("cuda", 0)
    box = torch.cuda.get_device_name(0)
    if args.only != "step":
        bench_kernel(args, box, dev)
    if args.only != "kernel":
        bench_step(args, box, dev)


if __name__ == "__main__":
    main()
