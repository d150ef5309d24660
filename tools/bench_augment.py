#!/usr/bin/env python
"""szn_augment_u8 (random scale / crop / flip, uint8 batch -> f32 network input + int64 target) at the shape a PASCAL batch has: B = 8,
500 x 500 canvas -> 512 x 512, scales over [0.5, 2]; against the kernel it replaces on the step path (szn_image_u8_to_bgr_f32 at B = 8,
512 x 512) and against a torch-on-device composition of the same operation (cast, interpolate, flip, pad, nearest for the labels).
HIP events around N launches after warm-up, the three alternating over R rounds; prints one JSON line."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zeroshotsemanticsegmentation_amd import _lib as L, datasets, utils

B, HM, WM, HO, WO, N, R, NREC = 8, 500, 500, 512, 512, 200, 5, 50
dev = torch.device("cuda")
g = torch.Generator(device="cuda"); g.manual_seed(1)
img = torch.randint(0, 256, (B, HM, WM, 3), device=dev, dtype=torch.uint8, generator=g)
lbl = torch.randint(-1, 33, (B, HM, WM), device=dev, dtype=torch.int64, generator=g)
img512 = torch.randint(0, 256, (B, HO, WO, 3), device=dev, dtype=torch.uint8, generator=g)
sizes = [(375, 500), (500, 375), (333, 500), (500, 500), (375, 500), (500, 334), (281, 500), (442, 500)]
aug = datasets.Augment((HO, WO), (0.5, 2.0))
recs_h = [aug.params(sizes, 0, it) for it in range(NREC)]                 # NREC draws, cycled; uploaded before the timed window
recs = [torch.from_numpy(r).to(dev) for r in recs_h]
mean = (C.c_double * 3)(*utils.MEAN_BGR)
mean_t = torch.tensor(utils.MEAN_BGR, device=dev, dtype=torch.float64).reshape(1, 3, 1, 1)
out = torch.empty(B, 3, HO, WO, device=dev); out_l = torch.empty(B, HO, WO, device=dev, dtype=torch.int64)


def run_augment(i):
    L.call("szn_augment_u8", B, HM, WM, L.ptr(img), L.ptr(lbl), L.ptr(recs[i % NREC]), mean, HO, WO, L.ptr(out), L.ptr(out_l), L.stream_ptr())


def run_plain(i):
    L.call("szn_image_u8_to_bgr_f32", B, HO, WO, L.ptr(img512), mean, L.ptr(out), L.stream_ptr())


def run_torch(i):
    for b, r in enumerate(recs_h[i % NREC]):
        h, w, Hs, Ws, _, _, oy, ox, flip = [int(v) for v in r]
        x = img[b, :h, :w].permute(2, 0, 1)[None].float()
        y = F.interpolate(x, size=(Hs, Ws), mode="bilinear", align_corners=False)[:, :, oy:oy + HO, ox:ox + WO]
        t = F.interpolate(lbl[b, :h, :w][None, None].float(), size=(Hs, Ws), mode="nearest")[:, :, oy:oy + HO, ox:ox + WO]
        y = (y.flip(1).double() - mean_t).float()
        ph, pw = HO - y.shape[2], WO - y.shape[3]
        y, t = F.pad(y, (0, pw, 0, ph)), F.pad(t, (0, pw, 0, ph), value=-2.0)
        if flip:
            y, t = y.flip(3), t.flip(3)
        out[b] = y[0]
        out_l[b] = t[0, 0].long()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(N):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / N * 1e3                                   # microseconds per launch


def needed_bytes(r):
    """what one launch has to move: 20 B per output pixel written, 3 + 8 B per source pixel under the crop window read once"""
    total = 20 * B * HO * WO
    for h, w, Hs, Ws, _, _, oy, ox, _ in [[int(v) for v in row] for row in r]:
        sh = min(h, -(-min(HO, Hs - oy) * h // Hs) + 1)
        sw = min(w, -(-min(WO, Ws - ox) * w // Ws) + 1)
        total += 11 * sh * sw
    return total


fns = {"augment_u8": run_augment, "image_u8_to_bgr_f32": run_plain, "torch_composition": run_torch}
for fn in fns.values():
    fn(0)
torch.cuda.synchronize()
us = {k: [] for k in fns}
for _ in range(R):
    for k, fn in fns.items():
        us[k].append(timed(fn))
res = {"shape": "B %d, canvas %dx%d -> %dx%d" % (B, HM, WM, HO, WO), "launches_per_round": N, "rounds": R}
for k, v in us.items():
    res[k + "_us"] = {"median": round(float(np.median(v)), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
nb = float(np.mean([needed_bytes(r) for r in recs_h]))
res["augment_bytes_needed_MB"] = round(nb / 1e6, 2)
res["augment_GBps"] = round(nb / (np.median(us["augment_u8"]) * 1e-6) / 1e9, 1)
res["augment_fraction_of_6.3TBps"] = round(res["augment_GBps"] / 6300.0, 3)
res["plain_GBps"] = round(15 * B * HO * WO / (np.median(us["image_u8_to_bgr_f32"]) * 1e-6) / 1e9, 1)
print(json.dumps(res))
