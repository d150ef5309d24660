#!/usr/bin/env python
"""The hubness correction of zero-shot inference (train.py --hub-correct: E = 300, K = 59), GPU only.  One JSON line per setting.

  head:    on a synthetic 1/32 map (stride 32) and 1/8 map (stride 8), 33 gammas, histograms and one prediction: one szn_hub_stats call, one
           szn_hub_head call on its table, and one szn_calib_head call on the same map, gammas and workspace size -- what the statistics
           pass costs, and what the fma and the two scalar loads per class cost the head.
  noacc:   with --noacc-lib: szn_hub_stats of a second build of the library whose pixel pass keeps the walk and the similarities and
           drops the quantisation, the reductions and the atomics -- what the reduction costs.  Build it with
             make -C zeroshotsemanticsegmentation_amd/csrc BUILD=build_exp LIB=../lib_exp/libszn_hip.so EXTRA=-DSZN_HUB_NO_ACCUM
  referee: szn_hub_stats + szn_hub_head for one gamma (prediction only) against utils.hub_infer for that gamma on a materialised (B,E,H,W)
           score of the same size (torch operations; the time to materialise it is not counted).
Per setting: warm-up, then --reps timed windows of device-event timing, the routes alternating window by window; median and min-max."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zeroshotsemanticsegmentation_amd import _lib as L, models, synth, utils  # noqa: E402
from bench_seen_sweep import UNSEEN, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--head-iters", type=int, default=10)
    ap.add_argument("--referee-iters", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--gammas", type=int, default=33)
    ap.add_argument("--mode", choices=sorted(L.HUB_MODES), default="zscore")
    ap.add_argument("--beta", type=float, default=1.0)
    ap.add_argument("--min-sd", type=float, default=0.05)
    ap.add_argument("--noacc-lib", default=None, help="a build of the library with -DSZN_HUB_NO_ACCUM")
    ap.add_argument("--no-referee", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hub: needs a GPU")
    lib, st = L.load(), L.stream_ptr()
    noacc = None
    if args.noacc_lib:
        noacc = C.CDLL(args.noacc_lib)
        noacc.szn_hub_stats.restype, noacc.szn_hub_stats.argtypes = L.SIGNATURES["szn_hub_stats"]
    dev = torch.device("cuda", 0)
    box = torch.cuda.get_device_name(0)
    H, E, K, B, N = args.size, 300, 59, args.batch, args.gammas
    mode = L.HUB_MODES[args.mode]
    emb = torch.from_numpy(synth.make_embeddings(K, E)).to(dev)
    unseen = L.class_set(UNSEEN)
    t = torch.from_numpy(synth.make_labels(B, H, H, K, seed=8)).to(dev)
    pred = torch.empty(B, H, H, dtype=torch.int64, device=dev)
    width = 0.5 if args.mode == "mean" else 2.0
    gammas = np.linspace(-width, width, N).astype(np.float32)
    gp = gammas.ctypes.data_as(C.POINTER(C.c_float))
    one = np.zeros(1, np.float32)
    op = one.ctypes.data_as(C.POINTER(C.c_float))
    hist = torch.zeros(N, K, K, dtype=torch.int64, device=dev)
    table = torch.empty(B, K, 2, device=dev)
    for S in (32, 8):
        crop = models.CROP if S == 32 else models.CROP_UP8
        h = (H + crop + S - 1) // S
        CP = (E + 2 + 63) // 64 * 64
        coarse = torch.zeros(B, h, h, CP, device=dev)
        coarse[..., :E] = torch.from_numpy(synth.uniform(7, (B, h, h, E), -2, 2)).to(dev)
        nbytes = lib.szn_hub_head_workspace_bytes(S, B, h, h, E, K, N)
        assert nbytes == lib.szn_calib_head_workspace_bytes(S, B, h, h, E, K, N)
        cws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        sws = torch.empty(lib.szn_hub_stats_workspace_bytes(S, B, h, h, E, K), dtype=torch.uint8, device=dev)

        def stats_args():
            return (S, B, h, h, E, CP, 0, H, H, crop, K, L.ptr(coarse), L.ptr(emb), L.ptr(t), mode, args.beta, args.min_sd, L.ptr(table),
                    None, None, L.ptr(sws), st)

        def stats():
            L.call("szn_hub_stats", *stats_args())

        def stats_noacc():
            assert noacc.szn_hub_stats(*stats_args()) == 0

        def hub():
            L.call("szn_hub_head", S, B, h, h, E, CP, 0, H, H, crop, K, L.ptr(coarse), L.ptr(emb), L.ptr(t), unseen, L.ptr(table), N, gp,
                   L.ptr(hist), N // 2, L.ptr(pred), L.ptr(cws), st)

        def calib():
            L.call("szn_calib_head", S, B, h, h, E, CP, 0, H, H, crop, K, L.ptr(coarse), L.ptr(emb), L.ptr(t), unseen, N, gp, L.ptr(hist), N // 2,
                   L.ptr(pred), L.ptr(cws), st)

        stats()                                     # the table the head reads
        routes = {"hub_stats": stats, "hub_head": hub, "calib_head": calib}
        if noacc is not None:
            routes["hub_stats_noacc"] = stats_noacc
        res = {"box": box, "what": "head", "stride": S, "B": B, "H": H, "W": H, "E": E, "K": K, "n_gammas": N, "mode": args.mode}
        res.update(timed(routes, args.reps, args.head_iters, args.warmup))
        res.update({"hub_over_calib": res["hub_head_ms"] / res["calib_head_ms"], "reps": args.reps, "iters": args.head_iters})
        print(json.dumps(res), flush=True)
        if noacc is not None:
            stats()                                 # (the variant leaves an identity table behind)
        if not args.no_referee:
            score = torch.randn(B, E, H, H, device=dev)
            valid = t != -2

            def hub_one():
                L.call("szn_hub_stats", *stats_args())
                L.call("szn_hub_head", S, B, h, h, E, CP, 0, H, H, crop, K, L.ptr(coarse), L.ptr(emb), None, unseen, L.ptr(table), 1, op,
                       None, 0, L.ptr(pred), L.ptr(cws), st)

            def referee():
                utils.hub_infer(score, emb, UNSEEN, args.mode, args.beta, 0.0, args.min_sd, valid)

            res = {"box": box, "what": "referee", "stride": S, "B": B, "H": H, "W": H, "E": E, "K": K, "n_gammas": 1, "mode": args.mode}
            res.update(timed({"hub_stats_and_head": hub_one, "hub_infer": referee}, args.reps, args.referee_iters, args.warmup))
            res.update({"infer_over_hub": res["hub_infer_ms"] / res["hub_stats_and_head_ms"], "reps": args.reps, "iters": args.referee_iters})
            print(json.dumps(res), flush=True)
            del score
        del coarse, cws, sws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
