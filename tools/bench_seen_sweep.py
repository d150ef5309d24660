#!/usr/bin/env python
"""The seen-mask threshold sweep of full SZN inference (train.py -m test_all --seen-threshold / --seen-sweep: E = 300, K = 59), GPU only.
One JSON line per setting.

  head:   on a synthetic 1/32 map (stride 32) and 1/8 map (stride 8, the seen-mask channels on their own 1/32 map, FCN8s' geometry), for
          N in {1, 33, 64} thresholds: szn_seenmask_margin + one szn_seen_sweep_head call (N histograms and one prediction) against the
          route the kernels before it allow, once per threshold: szn_seenmask_head_k pred-only, szn_fused_head_grouped (group mode 1),
          szn_confusion_hist_k.
  model:  one validation batch of the full network, FCN32s and FCN8s, bf16: szn_predict (plain test_all) against seen_sweep_predict
          with the single threshold 0 (--seen-threshold 0) and with a 33-tau sweep (--seen-sweep).
Per setting: warm-up, then --reps timed windows of device-event timing, the routes alternating window by window; median and min-max."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zeroshotsemanticsegmentation_amd import _lib as L, models, synth  # noqa: E402

UNSEEN = [0, 12, 16, 18]           # the Context 31/2/2 split's unseen classes (configs.py)


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


def bench_head(args, box, dev):
    H, E, K, B = args.size, 300, 59, args.batch
    lib, st = L.load(), L.stream_ptr()
    emb = torch.from_numpy(synth.make_embeddings(K, E)).to(dev)
    unseen = L.class_set(UNSEEN)
    h32 = (H + models.CROP + 31) // 32
    # a smooth seen-mask map, as the learned head gives: the 2-channel 1/32 map under a (2,2,64,64) filter bank
    sm = torch.from_numpy(synth.uniform(5, (B, h32, h32, 2), -1, 1)).to(dev)
    up_w = torch.from_numpy(synth.uniform(6, (2, 2, 64, 64), -0.1, 0.1)).to(dev)
    t = torch.from_numpy(synth.make_labels(B, H, H, K, seed=8)).to(dev)
    margin = torch.empty(B, H, H, device=dev)
    gmap = torch.empty(B, H, H, dtype=torch.int64, device=dev)
    pred = torch.empty(B, H, H, dtype=torch.int64, device=dev)
    conf = torch.zeros(3, K, K, dtype=torch.int64, device=dev)
    sws = torch.empty(lib.szn_seenmask_head_workspace_bytes(B, h32, h32, H, H, models.CROP), dtype=torch.uint8, device=dev)
    L.call("szn_seenmask_margin", B, h32, h32, 2, 0, H, H, models.CROP, L.ptr(sm), L.ptr(up_w), L.ptr(margin), st)
    torch.cuda.synchronize()
    lo, hi = float(margin.min()), float(margin.max())
    for S in (32, 8):
        crop = models.CROP if S == 32 else models.CROP_UP8
        h = (H + crop + S - 1) // S
        CP = (E + 2 + 63) // 64 * 64
        coarse = torch.zeros(B, h, h, CP, device=dev)
        coarse[..., :E] = torch.from_numpy(synth.uniform(7, (B, h, h, E), -2, 2)).to(dev)
        fws = torch.empty(lib.szn_fused_head_workspace_bytes(B, h, h, E, K), dtype=torch.uint8, device=dev)
        for N in (1, 33, 64):
            taus = np.linspace(lo / 2, hi / 2, N).astype(np.float32) if N > 1 else np.zeros(1, np.float32)
            tp = taus.ctypes.data_as(C.POINTER(C.c_float))
            hist = torch.zeros(N, K, K, dtype=torch.int64, device=dev)
            cws = torch.empty(lib.szn_seen_sweep_head_workspace_bytes(S, B, h, h, E, K, N), dtype=torch.uint8, device=dev)

            def one_pass():
                L.call("szn_seenmask_margin", B, h32, h32, 2, 0, H, H, models.CROP, L.ptr(sm), L.ptr(up_w), L.ptr(margin), st)
                L.call("szn_seen_sweep_head", S, B, h, h, E, CP, 0, H, H, crop, K, L.ptr(coarse), L.ptr(emb), L.ptr(t), unseen,
                       L.ptr(margin), N, tp, L.ptr(hist), N // 2, L.ptr(pred), L.ptr(cws), st)

            def looped():
                for _ in range(N):
                    L.call("szn_seenmask_head_k", B, h32, h32, 2, 0, H, H, models.CROP, L.ptr(sm), L.ptr(up_w), None, 0, None, None, None,
                           None, L.ptr(gmap), None, None, L.ptr(sws), st)
                    L.call("szn_fused_head_grouped", S, B, h, h, E, CP, 0, H, H, crop, K, L.ptr(coarse), L.ptr(emb), None, unseen, 1,
                           L.ptr(gmap), None, None, L.ptr(pred), L.SZN_F32, None, L.ptr(fws), st)
                    L.call("szn_confusion_hist_k", t.numel(), K, L.ptr(t), L.ptr(pred), None, L.ptr(conf), st)

            res = {"box": box, "what": "head", "stride": S, "B": B, "H": H, "W": H, "E": E, "K": K, "n_taus": N}
            res.update(timed({"one_pass": one_pass, "looped": looped}, args.reps, args.head_iters if N == 1 else max(1, args.head_iters // 4),
                             args.warmup))
            res.update({"looped_over_one_pass": res["looped_ms"] / res["one_pass_ms"], "reps": args.reps})
            print(json.dumps(res), flush=True)
        del coarse, fws
        torch.cuda.empty_cache()


def bench_model(args, box, dev):
    H, E, K, B = args.size, 300, 59, args.batch
    emb = torch.from_numpy(synth.make_embeddings(K, E)).to(dev)
    x = torch.from_numpy(synth.make_images(B, H, H, seed=11)).to(dev)
    t = torch.from_numpy(synth.make_labels(B, H, H, K, seed=13)).to(dev)
    sweep = np.linspace(-2, 2, 33).astype(np.float32)
    for arch, cls in (("fcn32s", models.FCN32s), ("fcn8s", models.FCN8s)):
        m = cls(E).load_synthetic(1337, device=dev).eval()
        m.set_precision(torch.bfloat16)
        hist = torch.zeros(33, K, K, dtype=torch.int64, device=dev)
        res = {"box": box, "what": "model", "arch": arch, "B": B, "H": H, "W": H, "E": E, "K": K, "precision": "bf16"}
        res.update(timed({"test_all": lambda: m.szn_predict(x, emb, UNSEEN, t),
                          "seen_threshold_0": lambda: m.seen_sweep_predict(x, emb, UNSEEN, [0.0], t, pred_index=0),
                          "seen_sweep_33": lambda: m.seen_sweep_predict(x, emb, UNSEEN, sweep, t, hist=hist, pred_index=16)},
                         args.reps, args.step_iters, args.warmup))
        res.update({"threshold_over_test_all": res["seen_threshold_0_ms"] / res["test_all_ms"],
                    "sweep_over_test_all": res["seen_sweep_33_ms"] / res["test_all_ms"], "reps": args.reps, "iters": args.step_iters})
        print(json.dumps(res), flush=True)
        del m
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--head-iters", type=int, default=20)
    ap.add_argument("--step-iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--only", choices=["head", "model"], default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_seen_sweep: needs a GPU")
    L.load()
    dev = torch.device("cuda", 0)
    box = torch.cuda.get_device_name(0)
    if args.only != "model":
        bench_head(args, box, dev)
    if args.only != "head":
        bench_model(args, box, dev)


if __name__ == "__main__":
    main()
