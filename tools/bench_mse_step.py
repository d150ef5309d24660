#!/usr/bin/env python
"""The MSE embedding configuration (train.py -loss mse: E = 300, K = 59, Adam), GPU only.  One JSON line per setting.

  head:  szn_fused_mse_head (coarse -> loss, pred, d coarse) against the five-kernel chain szn_bilinear_up_crop_fwd -> szn_mse_loss_fwd
         -> szn_embed_argmax_k -> szn_mse_loss_bwd -> szn_bilinear_up_crop_bwd on the same map; 512 x 512, B = 1 / 8, stride 32 (the 1/32
         map) and stride 8 (FCN8s' 1/8 fused map); the cosine fused head on the same inputs as a yardstick (what building P_k costs).
  step:  TrainStep(loss="mse") against the autograd route -loss mse ran before it (forward, utils.mse_loss, infer_lbl_device, backward,
         per-tensor FusedAdam), 512 x 512, B = 1 / 8, fp32 / bf16, train mode; the cosine TrainStep of the same process and precision
         as a yardstick.
Per setting: warm-up, then --reps timed windows of device-event timing, the routes alternating window by window; median and
min-max."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zeroshotsemanticsegmentation_amd import _lib as L, engine, models, optim, synth, utils  # noqa: E402


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
    H, E, K = args.size, 300, 59
    CP = (E + 2 + 63) // 64 * 64
    st = L.stream_ptr()
    emb = torch.from_numpy(synth.make_embeddings(K, E)).to(dev)
    for S, B in [(S, int(v)) for S in (32, 8) for v in args.batches.split(",")]:
        crop = models.CROP if S == 32 else models.CROP_UP8
        h = w = (H + crop + S - 1) // S
        coarse = torch.zeros(B, h, w, CP, device=dev)
        coarse[..., :E] = torch.from_numpy(synth.uniform(7, (B, h, w, E), -2, 2)).to(dev)
        t = torch.from_numpy(synth.make_labels(B, H, H, K, seed=8)).to(dev)
        score, dscore = torch.empty(B, E, H, H, device=dev), torch.empty(B, E, H, H, device=dev)
        lws = torch.empty(L.load().szn_loss_workspace_bytes(B, H, H), dtype=torch.uint8, device=dev)
        loss, stats = torch.empty(1, device=dev), torch.empty(B, 2, device=dev)
        pred = torch.empty(B, H, H, dtype=torch.int64, device=dev)
        dc = torch.zeros(B, h, w, CP, device=dev)
        fws = torch.empty(L.load().szn_fused_head_workspace_bytes(B, h, w, E, K), dtype=torch.uint8, device=dev)
        L.call("szn_fused_head_prepare", E, K, L.ptr(emb), L.ptr(fws), st)

        def chain():
            L.call("szn_bilinear_up_crop_fwd", S, B, h, w, E, CP, 0, H, H, crop, L.ptr(coarse), L.ptr(score), st)
            L.call("szn_mse_loss_fwd", B, E, H, H, K, L.ptr(score), L.ptr(t), L.ptr(emb), None, L.ptr(loss), L.ptr(stats), L.ptr(lws), st)
            L.call("szn_embed_argmax_k", B, E, H, H, K, L.ptr(score), L.ptr(emb), 0, None, None, None, L.ptr(pred), st)
            L.call("szn_mse_loss_bwd", B, E, H, H, K, L.ptr(score), L.ptr(t), L.ptr(emb), None, L.ptr(stats), None, L.ptr(dscore), st)
            L.call("szn_bilinear_up_crop_bwd", S, B, h, w, E, CP, 0, H, H, crop, L.ptr(dscore), L.ptr(dc), st)

        def fused(fn):
            L.call(fn, S, B, h, w, E, CP, 0, H, H, crop, K, L.ptr(coarse), L.ptr(emb), L.ptr(t), None, 0, None, L.ptr(loss),
                   L.ptr(stats), L.ptr(pred), L.SZN_F32, L.ptr(dc), L.ptr(fws), st)

        res = {"box": box, "what": "head", "stride": S, "B": B, "H": H, "W": H, "E": E, "K": K}
        res.update(timed({"chain": chain, "fused_mse": lambda: fused("szn_fused_mse_head_prepared"),
                          "fused_cos": lambda: fused("szn_fused_head_grouped_prepared")}, args.reps, args.head_iters, args.warmup))
        res.update({"speedup": res["chain_ms"] / res["fused_mse_ms"], "mse_over_cos": res["fused_mse_ms"] / res["fused_cos_ms"],
                    "score_bytes": B * E * H * H * 4, "reps": args.reps, "iters": args.head_iters})
        print(json.dumps(res), flush=True)
        del score, dscore, coarse, t, dc, fws, lws
        torch.cuda.empty_cache()


def bench_step(args, box, dev):
    H, E, K = args.size, 300, 59
    emb = synth.make_embeddings(K, E)
    for prec_name in args.precisions.split(","):
        prec = {"fp32": torch.float32, "bf16": torch.bfloat16}[prec_name]
        for B in [int(v) for v in args.batches.split(",")]:
            x = torch.from_numpy(synth.make_images(B, H, H, seed=11)).to(dev)
            t = torch.from_numpy(synth.make_labels(B, H, H, K, seed=13)).to(dev)
            mm = models.FCN32s(E).load_synthetic(1337, device=dev).train()
            mse = engine.TrainStep(mm, emb, loss="mse", optimizer="adam", lr=1e-5, precision=prec, keep_grads=False)
            # the autograd route train.py -loss mse took before: forward, mse_loss, class assignment, backward, per-tensor FusedAdam
            ma = models.FCN32s(E).load_synthetic(1337, device=dev).train()
            ma.set_precision(prec)
            layers = models.opt_layers(ma)
            opt = optim.FusedAdam([{"params": [getattr(ma, n).weight for n in layers]},
                                   {"params": [getattr(ma, n).bias for n in layers], "lr": 2e-5}], lr=1e-5)
            embt = torch.from_numpy(emb).to(dev)
            mk = models.FCN32s(E).load_synthetic(1337, device=dev).train()
            cos = engine.TrainStep(mk, emb, optimizer="adam", lr=1e-5, precision=prec, keep_grads=False)

            def autograd_step():
                score = ma(x, mode="fcn")
                loss = utils.mse_loss(score, t, embt)
                utils.infer_lbl_device(score.detach(), embt)
                opt.zero_grad()
                loss.backward()
                engine.allreduce_param_grads([p for g in opt.param_groups for p in g["params"]])
                opt.step()

            res = {"box": box, "what": "step", "B": B, "H": H, "W": H, "E": E, "K": K, "precision": prec_name}
            res.update(timed({"mse_trainstep": lambda: mse.step(x, t), "autograd": autograd_step, "cos_trainstep": lambda: cos.step(x, t)},
                             args.reps, args.step_iters, args.warmup))
            res.update({"speedup_vs_autograd": res["autograd_ms"] / res["mse_trainstep_ms"],
                        "mse_over_cos": res["mse_trainstep_ms"] / res["cos_trainstep_ms"], "reps": args.reps, "iters": args.step_iters})
            print(json.dumps(res), flush=True)
            del mse, mm, ma, opt, cos, mk, x, t
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
        raise SystemExit("bench_mse_step: needs a GPU")
    L.load()
    dev = torch.device("cuda", 0)
    box = torch.cuda.get_device_name(0)
    if args.only != "step":
        bench_head(args, box, dev)
    if args.only != "head":
        bench_step(args, box, dev)


if __name__ == "__main__":
    main()
