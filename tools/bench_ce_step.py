#!/usr/bin/env python
"""The softmax cross-entropy configuration (train.py -c 1: 21 classes, CE sum, SGD), GPU only.  One JSON line per setting.

  head:  szn_fused_ce_head (coarse -> loss, pred, d coarse) against the materialised chain szn_bilinear_up_crop_fwd -> szn_ce2d_fwd
         -> szn_ce2d_bwd -> szn_bilinear_up_crop_bwd on the same 1/32 map; 512 x 512, stride 32, B = 1 / 8, C = 21 / 59; algorithmic
         bytes of both routes and their time at 8 TB/s.
  step:  the cross-entropy TrainStep against the autograd route -c 1 ran before it (forward, utils.cross_entropy2d, backward,
         FusedSGD), 512 x 512, B = 1 / 8, fp32 / bf16, train mode; the cosine TrainStep (E = 300, K = 59, Adam) of the same process
         and precision as a yardstick.
Per setting: warm-up, then --reps timed windows of device-event timing, the routes alternating window by window; median and
min-max."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zeroshotsemanticsegmentation_amd import _lib as L, engine, models, synth, utils  # noqa: E402
from zeroshotsemanticsegmentation_amd.configs import configurations  # noqa: E402
from zeroshotsemanticsegmentation_amd.train import make_fcn_optimizer  # noqa: E402


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
    H = args.size
    S, crop = 32, models.CROP
    h = w = (H + crop + S - 1) // S
    st = L.stream_ptr()
    for C in (21, 59):
        CP = (C + 2 + 63) // 64 * 64
        for B in [int(v) for v in args.batches.split(",")]:
            coarse = torch.zeros(B, h, w, CP, device=dev)
            coarse[..., :C] = torch.from_numpy(synth.uniform(7 + C, (B, h, w, C), -4, 4)).to(dev)
            t = torch.from_numpy(synth.make_labels(B, H, H, C, seed=8)).to(dev)
            score, dscore = torch.empty(B, C, H, H, device=dev), torch.empty(B, C, H, H, device=dev)
            lws = torch.empty(L.load().szn_loss_workspace_bytes(B, H, H), dtype=torch.uint8, device=dev)
            loss, stats = torch.empty(1, device=dev), torch.empty(B, 2, device=dev)
            pred = torch.empty(B, H, H, dtype=torch.int64, device=dev)
            dc = torch.zeros(B, h, w, CP, device=dev)
            fws = torch.empty(L.load().szn_fused_ce_head_workspace_bytes(S, B, h, w, C), dtype=torch.uint8, device=dev)

            def chain():
                L.call("szn_bilinear_up_crop_fwd", S, B, h, w, C, CP, 0, H, H, crop, L.ptr(coarse), L.ptr(score), st)
                L.call("szn_ce2d_fwd", B, C, H, H, L.ptr(score), L.ptr(t), None, 0, L.ptr(loss), L.ptr(stats), L.ptr(pred), L.ptr(lws), st)
                L.call("szn_ce2d_bwd", B, C, H, H, L.ptr(score), L.ptr(t), None, 0, L.ptr(stats), None, L.ptr(dscore), st)
                L.call("szn_bilinear_up_crop_bwd", S, B, h, w, C, CP, 0, H, H, crop, L.ptr(dscore), L.ptr(dc), st)

            def fused():
                L.call("szn_fused_ce_head", S, B, h, w, C, CP, 0, H, H, crop, L.ptr(coarse), L.ptr(t), None, 0, L.ptr(loss),
                       L.ptr(stats), L.ptr(pred), L.SZN_F32, L.ptr(dc), L.ptr(fws), st)

            res = {"box": box, "what": "head", "stride": S, "B": B, "H": H, "W": H, "C": C}
            res.update(timed({"chain": chain, "fused": fused}, args.reps, args.head_iters, args.warmup))
            px, sc, cm = B * H * H, B * C * H * H * 4, B * h * w * C * 4
            # chain: score written, read by ce fwd and bwd, dscore written and read; labels read twice, pred written
            bytes_chain = 5 * sc + px * (8 + 8 + 8) + 2 * cm
            bytes_fused = px * (8 + 8) + 2 * cm + fws.numel() // 4          # labels, pred, coarse + dcoarse, cell tables (approx.)
            res.update({"bytes_chain": bytes_chain, "bytes_fused": bytes_fused, "chain_ms_at_8TBs": bytes_chain / 8e9,
                        "fused_ms_at_8TBs": bytes_fused / 8e9, "speedup": res["chain_ms"] / res["fused_ms"],
                        "reps": args.reps, "iters": args.head_iters})
            print(json.dumps(res), flush=True)
            del score, dscore, coarse, t, dc, fws, lws
            torch.cuda.empty_cache()


def bench_step(args, box, dev):
    H = args.size
    cfg = configurations[1]
    for prec_name in args.precisions.split(","):
        prec = {"fp32": torch.float32, "bf16": torch.bfloat16}[prec_name]
        for B in [int(v) for v in args.batches.split(",")]:
            x = torch.from_numpy(synth.make_images(B, H, H, seed=11)).to(dev)
            t21 = torch.from_numpy(synth.make_labels(B, H, H, 21, seed=12)).to(dev)
            t59 = torch.from_numpy(synth.make_labels(B, H, H, 59, seed=13)).to(dev)
            # the CE TrainStep (the trainer's wiring of configs[0])
            mc = models.FCN32s(21).load_synthetic(1337, device=dev).train()
            ce = engine.TrainStep(mc, None, loss="cross_entropy", optimizer="sgd", lr=cfg["fcn_lr"], momentum=0.99, weight_decay=0.0005,
                                  precision=prec, keep_grads=False)
            # the autograd route train.py -c 1 took before: forward, cross_entropy2d, backward, per-tensor FusedSGD
            ma = models.FCN32s(21).load_synthetic(1337, device=dev).train()
            ma.set_precision(prec)
            opt = make_fcn_optimizer(ma, cfg)
            # the cosine TrainStep of the flagship configuration as a yardstick
            mk = models.FCN32s(300).load_synthetic(1337, device=dev).train()
            cos = engine.TrainStep(mk, synth.make_embeddings(59, 300), optimizer="adam", lr=1e-5, precision=prec, keep_grads=False)

            def ce_step():
                ce.step(x, t21)

            def autograd_step():
                score = ma(x, mode="fcn")
                loss = utils.cross_entropy2d(score, t21, size_average=False)
                opt.zero_grad()
                loss.backward()
                engine.allreduce_param_grads([p for g in opt.param_groups for p in g["params"]])
                opt.step()

            def cos_step():
                cos.step(x, t59)

            res = {"box": box, "what": "step", "B": B, "H": H, "W": H, "C": 21, "precision": prec_name}
            res.update(timed({"ce_trainstep": ce_step, "autograd": autograd_step, "cos_trainstep": cos_step}, args.reps,
                             args.step_iters, args.warmup))
            res.update({"speedup_vs_autograd": res["autograd_ms"] / res["ce_trainstep_ms"],
                        "ce_over_cos": res["ce_trainstep_ms"] / res["cos_trainstep_ms"], "reps": args.reps, "iters": args.step_iters})
            print(json.dumps(res), flush=True)
            del ce, mc, ma, opt, cos, mk, x, t21, t59
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--head-iters", type=int, default=20)
    ap.add_argument("--step-iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--precisions", default="fp32,bf16")
    ap.add_argument("--only", choices=["head", "step"], default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ce_step: needs a GPU")
    L.load()
    dev = torch.device("cuda", 0)
    box = torch.cuda.get_device_name(0)
    if args.only != "step":
        bench_head(args, box, dev)
    if args.only != "head":
        bench_step(args, box, dev)


if __name__ == "__main__":
    main()
