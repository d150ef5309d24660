#!/usr/bin/env python
"""Class-prototype pooling (szn_class_proto) at B = 8, 512 x 512, E = 300, K = 59, GPU only.  One JSON line per stride and mode
(DESIGN.md section 7q).

  fused:         szn_class_proto -- all of it: the Gram table (unit mode), the cell pass over the labels, gather, the T^t x coarse
                 reduction, finalize -- on the synthetic maps of the sizes the backbones give (17 x 17 at stride 32, 74 x 74 at stride 8):
                 a class embedding per coarse position, scaled and noised; labels in 16 x 16 blocks of one class, the first rows unlabelled.
  materialised:  the only route without it: szn_bilinear_up_crop_fwd writes the (B,E,H,W) score (2.5 GB), torch divides by the norm over
                 the channels (unit mode), gathers the labelled pixels and index_add_s them per class into a float64 (K,E) table.
Per setting: warm-up, then --reps timed windows of HIP-event timing, the two routes alternating window by window; median and min-max.
The two routes' results are compared (largest difference over the largest entry) before anything is timed."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zeroshotsemanticsegmentation_amd import _lib as L, heads  # noqa: E402

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--mat-iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--modes", nargs="+", choices=["unit", "raw"], default=["unit", "raw"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_proto: needs a GPU")
    lib = L.load()
    dev = torch.device("cuda", 0)
    box = torch.cuda.get_device_name(0)
    B, H = args.batch, args.size
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    emb = torch.randn(K, E, device=dev, generator=gen)
    lbl = blocks(B, H, H, gen, dev)
    ok = ((lbl >= 0) & (lbl < K)).reshape(-1)
    idx = lbl.reshape(-1)[ok]
    for stride in (32, 8):
        h = w = coarse_size(H, stride)
        cls = torch.randint(0, K, (B, h, w), device=dev, generator=gen)
        cmap = (emb[cls] * (0.5 + torch.rand(B, h, w, 1, device=dev, generator=gen))
                + 0.6 * emb.norm(dim=1).mean() / E ** 0.5 * torch.randn(B, h, w, E, device=dev, generator=gen)).contiguous()
        crop = heads._CROP[stride]
        nbytes = lib.szn_class_proto_workspace_bytes(stride, B, h, w, E, K)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        sums = torch.empty(K, E, dtype=torch.float64, device=dev)
        counts = torch.empty(K, 2, dtype=torch.int64, device=dev)
        score = torch.empty(B, E, H, H, dtype=torch.float32, device=dev)
        msums = torch.zeros(K, E, dtype=torch.float64, device=dev)
        st = L.stream_ptr()
        for mode in args.modes:
            code = heads.proto_mode(mode)

            def run_fused():
                L.call("szn_class_proto", stride, B, h, w, E, E, 0, H, H, crop, K, L.ptr(cmap), L.ptr(lbl), None, code, 0, L.ptr(sums),
                       L.ptr(counts), L.ptr(ws), st)

            def run_mat():
                L.call("szn_bilinear_up_crop_fwd", stride, B, h, w, E, E, 0, H, H, crop, L.ptr(cmap), L.ptr(score), st)
                v = score / score.norm(dim=1, keepdim=True) if mode == "unit" else score
                v = v.permute(0, 2, 3, 1).reshape(-1, E)[ok]
                msums.zero_()
                msums.index_add_(0, idx, v.double())

            run_fused()
            run_mat()
            torch.cuda.synchronize()
            diff = float((sums - msums).abs().max() / msums.abs().max())
            res = {"box": box, "what": "class_proto", "stride": stride, "mode": mode, "map": [h, w], "B": B, "H": H, "W": H, "E": E, "K": K,
                   "workspace_mb": nbytes / 2 ** 20, "score_mb": score.numel() * 4 / 2 ** 20, "pixels": int(counts[:, 0].sum()),
                   "contributing": int(counts[:, 1].sum()), "max_diff_over_max": diff}
            t = timed({"fused": run_fused}, args.reps, args.iters, args.warmup)
            # the two routes alternating window by window, at the slower route's iteration count
            t2 = timed({"fused": run_fused, "materialised": run_mat}, args.reps, args.mat_iters, 1)
            res.update({"fused_ms": t["fused_ms"], "fused_ms_minmax": t["fused_ms_minmax"], "fused_alt_ms": t2["fused_ms"],
                        "materialised_ms": t2["materialised_ms"], "materialised_ms_minmax": t2["materialised_ms_minmax"],
                        "materialised_over_fused": t2["materialised_ms"] / t2["fused_ms"], "reps": args.reps, "iters": args.iters,
                        "mat_iters": args.mat_iters})
            print(json.dumps(res), flush=True)
        del cmap, ws, score
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
