#!/usr/bin/env python
"""Self-training pseudo labels (szn_pseudo_head, TrainStep(pseudo=)) at B = 8, 512 x 512, E = 300, K = 59, bf16, GPU only.  One JSON
line per setting.

  head:  szn_pseudo_head -- all of it: embedding tables, clearing the histogram, the pixel pass, thresholds, relabel -- against
         szn_calib_head with one gamma and the prediction only (the cheapest call that evaluates the same per-pixel rule), on the same
         synthetic maps of the sizes the backbones give (17 x 17 at stride 32, 74 x 74 at stride 8).  The maps and labels are
         tools/bench_calib.py's: a class embedding per coarse position, scaled and noised; labels in 16 x 16 blocks of one class, with
         the pixels of one third of the classes -- the unseen ones -- hidden.
  step:  the whole TrainStep (cosine and sim_ce) with pseudo labels active against the same step built with pseudo=None, on the same
         images and the same hidden labels.
Per setting: warm-up, then --reps timed windows of HIP-event timing, the routes alternating window by window; median and min-max."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zeroshotsemanticsegmentation_amd import _lib as L, datasets, engine, heads, models, synth  # noqa: E402

E, K = 300, 59
UNSEEN = list(range(2, K, 3))                 # one third of the classes, bench_calib.py's set


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


def coarse_size(n, stride):
    m = n + 198
    for _ in range(5):
        m = (m + 1) // 2
    m -= 6
    return m if stride == 32 else 4 * m + 6


def hidden_blocks(B, H, W, gen, dev):
    """16 x 16 blocks of one class, the first rows unlabelled, the unseen classes' pixels hidden"""
    t = torch.randint(0, K, (B, H // 16, W // 16), device=dev, generator=gen).repeat_interleave(16, 1).repeat_interleave(16, 2)
    t[:, :8, :] = -1
    t[torch.isin(t, torch.tensor(UNSEEN, device=dev))] = datasets.HIDDEN_LABEL
    return t.contiguous()


def bench_head(args, box, dev):
    B, H = args.batch, args.size
    lib = L.load()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    emb = torch.randn(K, E, device=dev, generator=gen)
    tgt = hidden_blocks(B, H, H, gen, dev)
    unseen = L.class_set(UNSEEN)
    gamma = np.zeros(1, dtype=np.float32)
    gp = gamma.ctypes.data_as(C.POINTER(C.c_float))
    for stride in (32, 8):
        h = w = coarse_size(H, stride)
        cls = torch.randint(0, K, (B, h, w), device=dev, generator=gen)
        cmap = (emb[cls] * (0.5 + torch.rand(B, h, w, 1, device=dev, generator=gen))
                + 0.6 * emb.norm(dim=1).mean() / E ** 0.5 * torch.randn(B, h, w, E, device=dev, generator=gen)).contiguous()
        crop = heads._CROP[stride]
        ws_c = torch.empty(lib.szn_calib_head_workspace_bytes(stride, B, h, w, E, K, 1), dtype=torch.uint8, device=dev)
        ws_p = torch.empty(lib.szn_pseudo_head_workspace_bytes(stride, B, h, w, E, K, H, H), dtype=torch.uint8, device=dev)
        pred = torch.empty(B, H, H, dtype=torch.int64, device=dev)
        out = torch.empty(B, H, H, dtype=torch.int64, device=dev)
        counts = torch.zeros(K, 2, dtype=torch.int64, device=dev)
        st = L.stream_ptr()

        def run_calib():
            L.call("szn_calib_head", stride, B, h, w, E, E, 0, H, H, crop, K, L.ptr(cmap), L.ptr(emb), None, unseen, 1, gp, None, 0,
                   L.ptr(pred), L.ptr(ws_c), st)

        def run_pseudo():
            L.call("szn_pseudo_head", stride, B, h, w, E, E, 0, H, H, crop, K, L.ptr(cmap), L.ptr(emb), L.ptr(tgt), unseen, 0.0,
                   args.floor, args.permille, datasets.HIDDEN_LABEL, L.ptr(out), None, None, None, None, L.ptr(counts), L.ptr(ws_p), st)

        res = {"box": box, "what": "head", "stride": stride, "map": [h, w], "B": B, "H": H, "W": H, "E": E, "K": K,
               "keep_permille": args.permille, "conf_floor": args.floor}
        res.update(timed({"pseudo": run_pseudo, "calib_pred": run_calib}, args.reps, args.head_iters, args.warmup))
        torch.cuda.synchronize()
        c = counts.cpu().numpy()
        res.update({"pseudo_over_calib_pred": res["pseudo_ms"] / res["calib_pred_ms"], "hidden_pixels": int((tgt == datasets.HIDDEN_LABEL).sum()),
                    "candidates": int(c[:, 0].sum()), "selected": int(c[:, 1].sum()), "reps": args.reps, "iters": args.head_iters})
        print(json.dumps(res), flush=True)
        del cmap, ws_c, ws_p
        torch.cuda.empty_cache()


def bench_step(args, box, dev):
    B, H = args.batch, args.size
    emb = synth.make_embeddings(K, E)
    x = torch.from_numpy(synth.make_images(B, H, H, seed=11)).to(dev)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(2)
    t = hidden_blocks(B, H, H, gen, dev)
    cfg = dict(unseen=UNSEEN, gamma=args.gamma, keep=args.permille / 1000.0, conf_floor=args.floor)
    for loss in ("cos", "sim_ce"):
        kw = dict(sim_exclude=UNSEEN) if loss == "sim_ce" else {}
        steps = {}
        for name, pseudo in (("pseudo", cfg), ("plain", None)):
            m = models.FCN32s(E).load_synthetic(1337, device=dev).train()
            steps[name] = engine.TrainStep(m, emb, loss=loss, optimizer="adam", lr=1e-5, precision=torch.bfloat16, keep_grads=False,
                                           pseudo=pseudo, **kw)
        res = {"box": box, "what": "step", "loss": loss, "B": B, "H": H, "W": H, "E": E, "K": K, "precision": "bf16",
               "keep_permille": args.permille, "gamma": args.gamma, "conf_floor": args.floor}
        res.update(timed({"pseudo_step": lambda: steps["pseudo"].step(x, t), "plain_step": lambda: steps["plain"].step(x, t)},
                         args.reps, args.step_iters, args.warmup))
        c = steps["pseudo"].pseudo_counts.cpu().numpy()
        n_steps = (args.warmup + args.reps * args.step_iters)
        res.update({"extra_ms": res["pseudo_step_ms"] - res["plain_step_ms"], "pseudo_over_plain": res["pseudo_step_ms"] / res["plain_step_ms"],
                    "hidden_pixels": int((t == datasets.HIDDEN_LABEL).sum()), "candidates_per_step": float(c[:, 0].sum()) / n_steps,
                    "selected_per_step": float(c[:, 1].sum()) / n_steps, "reps": args.reps, "iters": args.step_iters})
        print(json.dumps(res), flush=True)
        del steps
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--head-iters", type=int, default=50)
    ap.add_argument("--step-iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--permille", type=int, default=300)
    ap.add_argument("--gamma", type=float, default=0.0)
    ap.add_argument("--floor", type=float, default=-2.0)
    ap.add_argument("--only", choices=["head", "step"], default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pseudo: needs a GPU")
    L.load()
    dev = torch.device("cuda", 0)
    box = torch.cuda.get_device_name(0)
    if args.only != "step":
        bench_head(args, box, dev)
    if args.only != "head":
        bench_step(args, box, dev)


if __name__ == "__main__":
    main()
