#!/usr/bin/env python
"""szn_augment_affine_u8 (rotation and colour jitter: a 2 x 3 position map and a 3 x 4 colour matrix per image) next to szn_augment_u8
(scale / crop / flip) in the same run, at the shape a PASCAL batch has: B = 8, 500 x 500 canvas -> 512 x 512.  Three records for the new
entry: the bridge of szn_augment_u8's own records with the identity colour (the same pixels, bit for bit), 10 degrees with the identity
colour, 10 degrees with a full jitter matrix.  HIP events around N launches after warm-up, the four alternating over R rounds; prints one
JSON line: microseconds, the ratio to szn_augment_u8 in this run and the bytes each launch has to move.  No gate."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zeroshotsemanticsegmentation_amd import _lib as L, datasets, utils

B, HM, WM, HO, WO, N, R, NREC = 8, 500, 500, 512, 512, 200, 5, 50
dev = torch.device("cuda")
g = torch.Generator(device="cuda"); g.manual_seed(1)
img = torch.randint(0, 256, (B, HM, WM, 3), device=dev, dtype=torch.uint8, generator=g)
lbl = torch.randint(-1, 33, (B, HM, WM), device=dev, dtype=torch.int64, generator=g)
sizes = [(375, 500), (500, 375), (333, 500), (500, 500), (375, 500), (500, 334), (281, 500), (442, 500)]
A = datasets.Augment
plain = A((HO, WO), (0.5, 2.0))
JITTER = A.color_matrix(0.1, 1.3, 0.6, 15.0)


def records(it, kind):
    """NREC draws of the plain augmentation (uploaded before the timed window), and the same draws as affine records of each kind"""
    p = plain.params(sizes, 0, it)
    if kind == "plain":
        return p
    out = np.empty((B, L.AUGA_NPARAM), dtype=np.int32)
    for i, (h, w) in enumerate(sizes):
        u = plain.draw(i, 0, it)
        s, flip = plain.scale[0] + (plain.scale[1] - plain.scale[0]) * u[0], bool(p[i, 8])
        if kind == "bridge":
            out[i] = A.affine_record(h, w, s, 0.0, u[1], u[2], flip, (HO, WO))
        else:
            out[i] = A.affine_record(h, w, s, 10.0 if i % 2 else -10.0, u[1], u[2], flip, (HO, WO), JITTER if kind == "rot10_jitter" else None)
    return out


KINDS = {"augment_u8": "plain", "affine_bridge": "bridge", "affine_rot10": "rot10", "affine_rot10_jitter": "rot10_jitter"}
recs_h = {k: [records(it, kind) for it in range(NREC)] for k, kind in KINDS.items()}
assert all(np.array_equal(a[:, :2], b[:, :2]) for a, b in zip(recs_h["augment_u8"], recs_h["affine_bridge"]))
recs = {k: [torch.from_numpy(r).to(dev) for r in v] for k, v in recs_h.items()}
mean = (C.c_double * 3)(*utils.MEAN_BGR)
out = torch.empty(B, 3, HO, WO, device=dev); out_l = torch.empty(B, HO, WO, device=dev, dtype=torch.int64)


def runner(k):
    entry = "szn_augment_u8" if k == "augment_u8" else "szn_augment_affine_u8"
    return lambda i: L.call(entry, B, HM, WM, L.ptr(img), L.ptr(lbl), L.ptr(recs[k][i % NREC]), mean, HO, WO, L.ptr(out), L.ptr(out_l),
                            L.stream_ptr())


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(N):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / N * 1e3                                   # microseconds per launch


def needed_bytes(k, i):
    """what one launch has to move: 20 B per output pixel written, 3 + 8 B per source pixel that some output pixel's nearest position names
    (counted on the host from the label plane of a launch with labels = the pixel's own index: exact for every kind)"""
    idx = torch.arange(HM * WM, device=dev, dtype=torch.int64).reshape(1, HM, WM).expand(B, HM, WM).contiguous()
    entry = "szn_augment_u8" if k == "augment_u8" else "szn_augment_affine_u8"
    L.call(entry, B, HM, WM, L.ptr(img), L.ptr(idx), L.ptr(recs[k][i]), mean, HO, WO, L.ptr(out), L.ptr(out_l), L.stream_ptr())
    src = sum(int(torch.unique(out_l[b][out_l[b] >= 0]).numel()) for b in range(B))
    return 20 * B * HO * WO + 11 * src


fns = {k: runner(k) for k in KINDS}
# the bridge is the same pixels
fns["augment_u8"](0)
ref_d, ref_l = out.clone(), out_l.clone()
fns["affine_bridge"](0)
assert torch.equal(out, ref_d) and torch.equal(out_l, ref_l), "the bridge record must reproduce szn_augment_u8 bit for bit"
for fn in fns.values():
    fn(0)
torch.cuda.synchronize()
us = {k: [] for k in fns}
for _ in range(R):
    for k, fn in fns.items():
        us[k].append(timed(fn))
res = {"shape": "B %d, canvas %dx%d -> %dx%d" % (B, HM, WM, HO, WO), "launches_per_round": N, "rounds": R}
base = float(np.median(us["augment_u8"]))
for k, v in us.items():
    med = float(np.median(v))
    nb = float(np.mean([needed_bytes(k, i) for i in range(0, NREC, 10)]))
    res[k] = {"us_median": round(med, 2), "us_min": round(min(v), 2), "us_max": round(max(v), 2), "ratio_to_augment_u8": round(med / base, 3),
              "bytes_needed_MB": round(nb / 1e6, 2), "GBps": round(nb / (med * 1e-6) / 1e9, 1)}
print(json.dumps(res))
