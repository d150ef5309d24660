#!/usr/bin/env python
"""bench_bf16x3.py -- the headline training step (FCN32s, B = 8, 512 x 512, E = 300, K = 59, fused head, Adam) at precision fp32,
bf16x3 and bf16 in one process.  Prints one JSON line: ms_per_step and Mpx/s per precision, and step_mfma_frac of bf16x3 against a
third of the bf16 matrix peak (each split product costs three bf16 products' worth of MFMA work in the paired form).

    python tools/bench_bf16x3.py [--batch 8] [--size 512] [--steps 10] [--warmup 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BF16 = 2500.0                     # TFLOP/s dense bf16 MFMA (MI355X)
STEP_MFLOP_PER_PX = {512: 4.342}       # phase-1 train step, E = 300 (bench.py)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--classes", type=int, default=59)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="fp32,bf16x3,bf16")
    args = ap.parse_args()
    import torch
    from zeroshotsemanticsegmentation_amd import _lib as L
    from zeroshotsemanticsegmentation_amd import engine, models, synth
    L.load()
    dev = torch.device("cuda", 0)
    B, H, K, E = args.batch, args.size, args.classes, 300
    emb = synth.make_embeddings(K, E)
    x = torch.from_numpy(synth.make_images(B, H, H, seed=1337)).to(dev)
    t = torch.from_numpy(synth.make_labels(B, H, H, K, seed=1337, classes=list(range(49)))).to(dev)
    prec = {"fp32": torch.float32, "bf16x3": "bf16x3", "bf16": torch.bfloat16}
    out = {"workload": "FCN32s train step, B=%d, %dx%d, E=%d, K=%d, fused head, Adam" % (B, H, H, E, K), "ms_per_step": {}, "Mpx_s": {},
           "loss": {}}
    for name in args.only.split(","):
        torch.manual_seed(1337)
        m = models.FCN32s(n_class=E)
        m.load_synthetic(1337, device=dev)
        m.train()
        ts = engine.TrainStep(m, emb, optimizer="adam", lr=1e-5, precision=prec[name], fused_head=True, keep_grads=False)
        for _ in range(args.warmup):
            loss, _ = ts.step(x, t)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            loss, _ = ts.step(x, t)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / args.steps
        out["ms_per_step"][name] = round(ms, 3)
        out["Mpx_s"][name] = round(B * H * H / (ms * 1e-3) / 1e6, 2)
        out["loss"][name] = round(float(loss), 6)
        del ts, m
        torch.cuda.empty_cache()
    mf = STEP_MFLOP_PER_PX.get(H)
    if mf and "bf16x3" in out["ms_per_step"]:
        ms = out["ms_per_step"]["bf16x3"]
        out["step_mfma_frac_bf16x3"] = round(mf * 1e6 * B * H * H / (ms * 1e-3) / 1e12 / (PEAK_BF16 / 3.0), 4)
    if "fp32" in out["ms_per_step"] and "bf16x3" in out["ms_per_step"]:
        out["speedup_bf16x3_vs_fp32"] = round(out["ms_per_step"]["fp32"] / out["ms_per_step"]["bf16x3"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
