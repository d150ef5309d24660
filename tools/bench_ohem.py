#!/usr/bin/env python
"""Hard-pixel mining (szn_ohem_head, TrainStep(ohem=)) at B = 8, 512 x 512, E = 300, K = 59, bf16, GPU only.  One JSON line per setting
(DESIGN.md section 7m).

  head:  szn_ohem_head -- all of it: embedding tables, clearing the histogram, the pixel pass, the cut, relabel -- against the two calls
         it sits between: szn_pseudo_head on the same map with one third of the classes hidden (K times the per-pixel arithmetic on a
         few percent of the pixels) and the fused cosine head itself (szn_fused_head_strided: loss, prediction and d(map)), on the
         synthetic maps of the sizes the backbones give (17 x 17 at stride 32, 74 x 74 at stride 8): a class embedding per coarse
         position, scaled and noised; labels in 16 x 16 blocks of one class, the first rows unlabelled.
  step:  the whole cosine TrainStep with ohem=dict(keep=KEEP) against the same step built with ohem=None, in one process, on the same
         images and labels.
Per setting: warm-up, then --reps timed windows of HIP-event timing, the routes alternating window by window; median and min-max."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zeroshotsemanticsegmentation_amd import _lib as L, datasets, engine, heads, models, synth  # noqa: E402

E, K = 300, 59
UNSEEN = list(range(2, K, 3))                 # the classes the pseudo-head comparison hides (tools/bench_pseudo.py's set)


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


def blocks(B, H, W, gen, dev):
    """16 x 16 blocks of one class, the first rows unlabelled"""
    t = torch.randint(0, K, (B, H // 16, W // 16), device=dev, generator=gen).repeat_interleave(16, 1).repeat_interleave(16, 2)
    t[:, :8, :] = -1
    return t.contiguous()


def bench_head(args, box, dev):
    B, H = args.batch, args.size
    lib = L.load()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    emb = torch.randn(K, E, device=dev, generator=gen)
    tgt = blocks(B, H, H, gen, dev)
    hidden = torch.where(torch.isin(tgt, torch.tensor(UNSEEN, device=dev)), torch.full_like(tgt, datasets.HIDDEN_LABEL), tgt)
    unseen = L.class_set(UNSEEN)
    for stride in (32, 8):
        h = w = coarse_size(H, stride)
        cls = torch.randint(0, K, (B, h, w), device=dev, generator=gen)
        cmap = (emb[cls] * (0.5 + torch.rand(B, h, w, 1, device=dev, generator=gen))
                + 0.6 * emb.norm(dim=1).mean() / E ** 0.5 * torch.randn(B, h, w, E, device=dev, generator=gen)).contiguous()
        crop = heads._CROP[stride]
        ws_o = torch.empty(lib.szn_ohem_head_workspace_bytes(stride, B, h, w, E, K, H, H), dtype=torch.uint8, device=dev)
        ws_p = torch.empty(lib.szn_pseudo_head_workspace_bytes(stride, B, h, w, E, K, H, H), dtype=torch.uint8, device=dev)
        ws_f = torch.empty(lib.szn_fused_head_workspace_bytes(B, h, w, E, K), dtype=torch.uint8, device=dev)
        pred = torch.empty(B, H, H, dtype=torch.int64, device=dev)
        out = torch.empty(B, H, H, dtype=torch.int64, device=dev)
        out_p = torch.empty(B, H, H, dtype=torch.int64, device=dev)
        counts = torch.zeros(B, 2, dtype=torch.int64, device=dev)
        qhist = torch.zeros(B, L.OHEM_BINS, dtype=torch.int64, device=dev)
        loss, stats = torch.empty(1, device=dev), torch.empty(B, 2, device=dev)
        dmap = torch.zeros_like(cmap)
        st = L.stream_ptr()

        def run_ohem():
            L.call("szn_ohem_head", stride, B, h, w, E, E, 0, H, H, crop, K, L.ptr(cmap), L.ptr(emb), L.ptr(tgt), None, args.permille,
                   args.thresh, heads.OHEM_DROP_LABEL, L.ptr(out), None, L.ptr(qhist), None, L.ptr(counts), L.ptr(ws_o), st)

        def run_pseudo():
            L.call("szn_pseudo_head", stride, B, h, w, E, E, 0, H, H, crop, K, L.ptr(cmap), L.ptr(emb), L.ptr(hidden), unseen, 0.0, -2.0,
                   300, datasets.HIDDEN_LABEL, L.ptr(out_p), None, None, None, None, None, L.ptr(ws_p), st)

        def run_head():
            L.call("szn_fused_head_strided", stride, B, h, w, E, E, 0, H, H, crop, K, L.ptr(cmap), L.ptr(emb), L.ptr(tgt), L.ptr(loss),
                   L.ptr(stats), L.ptr(pred), L.SZN_F32, L.ptr(dmap), L.ptr(ws_f), st)

        res = {"box": box, "what": "head", "stride": stride, "map": [h, w], "B": B, "H": H, "W": H, "E": E, "K": K,
               "keep_permille": args.permille, "thresh": args.thresh}
        res.update(timed({"ohem": run_ohem, "pseudo": run_pseudo, "cos_head": run_head}, args.reps, args.head_iters, args.warmup))
        torch.cuda.synchronize()
        c = counts.cpu().numpy()
        res.update({"ohem_over_pseudo": res["ohem_ms"] / res["pseudo_ms"], "ohem_over_cos_head": res["ohem_ms"] / res["cos_head_ms"],
                    "evaluated": int(c[:, 0].sum()), "kept": int(c[:, 1].sum()),
                    "bins_used_per_image": [int(v) for v in (qhist > 0).sum(dim=1).cpu().numpy()], "reps": args.reps,
                    "iters": args.head_iters})
        print(json.dumps(res), flush=True)
        del cmap, dmap, ws_o, ws_p, ws_f
        torch.cuda.empty_cache()


def bench_step(args, box, dev):
    B, H = args.batch, args.size
    emb = synth.make_embeddings(K, E)
    x = torch.from_numpy(synth.make_images(B, H, H, seed=11)).to(dev)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(2)
    t = blocks(B, H, H, gen, dev)
    cfg = dict(keep=args.permille / 1000.0, thresh=None if args.thresh <= -1 else args.thresh)
    steps = {}
    for name, ohem in (("ohem", cfg), ("plain", None)):
        m = models.FCN32s(E).load_synthetic(1337, device=dev).train()
        steps[name] = engine.TrainStep(m, emb, loss="cos", optimizer="adam", lr=1e-5, precision=torch.bfloat16, keep_grads=False,
                                       ohem=ohem)
    res = {"box": box, "what": "step", "loss": "cos", "B": B, "H": H, "W": H, "E": E, "K": K, "precision": "bf16",
           "keep_permille": args.permille, "thresh": args.thresh}
    res.update(timed({"ohem_step": lambda: steps["ohem"].step(x, t), "plain_step": lambda: steps["plain"].step(x, t)},
                     args.reps, args.step_iters, args.warmup))
    c = steps["ohem"].ohem_counts.cpu().numpy()
    n_steps = (args.warmup + args.reps * args.step_iters)
    res.update({"extra_ms": res["ohem_step_ms"] - res["plain_step_ms"], "ohem_over_plain": res["ohem_step_ms"] / res["plain_step_ms"],
                "evaluated_per_step": float(c[0]) / n_steps, "kept_per_step": float(c[1]) / n_steps, "reps": args.reps,
                "iters": args.step_iters})
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--head-iters", type=int, default=50)
    ap.add_argument("--step-iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--permille", type=int, default=250)
    ap.add_argument("--thresh", type=float, default=-2.0)
    ap.add_argument("--only", choices=["head", "step"], default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ohem: needs a GPU")
    L.load()
    dev = torch.device("cuda", 0)
    box = torch.cuda.get_device_name(0)
    if args.only != "step":
        bench_head(args, box, dev)
    if args.only != "head":
        bench_step(args, box, dev)


if __name__ == "__main__":
    main()
