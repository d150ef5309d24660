#!/usr/bin/env python
"""szn_ms_head (the view-ensemble embedding head) at B = 8, 512 x 512, E = 300, K = 59, scales {0.5, 0.75, 1, 1.25, 1.5} each with its
mirror image (10 views, synthetic coarse maps of the sizes the FCN32s backbone gives), against the route it replaces: per view
szn_bilinear_up_crop_fwd -> torch bilinear resize to 512 x 512 (mirrored back) -> cosine similarities added into a (B,K,H,W) accumulator,
then its argmax (torch: szn_embed_argmax takes a score and forms the similarities itself, it cannot take summed ones).  The replaced route
runs one image at a time (its (B,E,Hs,Ws) score of the 1.5 view alone is 5.7 GB).  HIP events around N_HEAD / N_OLD calls after warm-up, the
two routes alternating over R rounds; prints one JSON line with both times and the HBM bytes each route needs.
What the times include: ms_head_ms is the whole szn_ms_head call with every buffer allocated before the window (szn_fused_head_prepare,
one tables launch per view, the pixel kernel, and the host's argument marshalling between launches); replaced_ms includes torch's
allocations of the per-view scores, served by its caching allocator after the warm-up call."""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zeroshotsemanticsegmentation_amd import _lib as L, heads

B, H, W, E, K, S, R = 8, 512, 512, 300, 59, 32, 5
N_HEAD, N_OLD = 200, 3            # calls per timed window: a head call is short next to the replaced route, which moves gigabytes per call
SCALES = (0.5, 0.75, 1.0, 1.25, 1.5)
dev = torch.device("cuda")
g = torch.Generator(device="cuda"); g.manual_seed(1)


def coarse_size(n):
    m = n + 198
    for _ in range(5):
        m = (m + 1) // 2
    return m - 6


plan = heads.ms_views(H, W, SCALES, True)
maps = [torch.rand(B, coarse_size(Hs), coarse_size(Ws), E, device=dev, generator=g) + 0.5 for Hs, Ws, _ in plan]
emb = torch.randn(K, E, device=dev, generator=g)
views = [(m,) + v for m, v in zip(maps, plan)]


# the head's call with everything allocated once, outside the timed window (heads.ms_predict allocates per call)
arr = (L.MsView * len(views))()
for rec, (m, Hs, Ws, flip) in zip(arr, views):
    rec.coarse, rec.h, rec.w, rec.ldc, rec.c0, rec.Hs, rec.Ws, rec.flip = m.data_ptr(), m.shape[1], m.shape[2], m.shape[3], 0, Hs, Ws, int(flip)
ws = torch.empty(L.load().szn_ms_head_workspace_bytes(S, B, E, K, len(views), arr), dtype=torch.uint8, device=dev)
pred_head = torch.empty(B, H, W, dtype=torch.int64, device=dev)


def run_head():
    L.call("szn_ms_head", S, B, E, K, H, W, heads.CROP, len(views), arr, L.ptr(emb), None, 0, None, None, L.ptr(pred_head), None,
           L.ptr(ws), L.stream_ptr())
    return pred_head


en = emb.norm(dim=1).reshape(1, K, 1, 1)


def run_replaced():
    pred = torch.empty(B, H, W, dtype=torch.int64, device=dev)
    for b in range(B):
        acc = torch.zeros(1, K, H, W, device=dev)
        for m, Hs, Ws, flip in views:
            score = torch.empty(1, E, Hs, Ws, device=dev)
            mb = m[b:b + 1]
            L.call("szn_bilinear_up_crop_fwd", S, 1, mb.shape[1], mb.shape[2], E, E, 0, Hs, Ws, heads.CROP, L.ptr(mb), L.ptr(score),
                   L.stream_ptr())
            s = F.interpolate(score, size=(H, W), mode="bilinear", align_corners=False)
            if flip:
                s = s.flip(3)
            acc += torch.einsum("ke,behw->bkhw", emb, s) / (s.norm(dim=1, keepdim=True) * en)
        pred[b] = acc.argmax(1)[0]
    return pred


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


p_head, p_old = run_head().clone(), run_replaced()              # warm-up, and the two routes agree except near ties
agree = float((p_head == p_old).float().mean())
times = {"ms_head": [], "replaced": []}
for _ in range(R):
    times["ms_head"].append(timed(run_head, N_HEAD))
    times["replaced"].append(timed(run_replaced, N_OLD))
npos = [B * m.shape[1] * m.shape[2] for m in maps]
KP = 64
head_bytes = sum(n * E * 4 + 2 * n * (KP + 16) * 4 for n in npos) + B * H * W * 8 + (E * KP + 2 * KP) * 4
# replaced: per view the score written and read, the resized score written and read, the accumulator read and written; then the argmax
old_bytes = sum(B * E * Hs * Ws * 4 * 2 + B * E * H * W * 4 * 2 + B * K * H * W * 4 * 2 for _, Hs, Ws, _ in views) + B * K * H * W * 4 + B * H * W * 8
print(json.dumps({"shape": [B, H, W, E, K], "views": len(views), "calls_per_window": [N_HEAD, N_OLD],
                  "ms_head_ms": float(np.median(times["ms_head"])), "ms_head_ms_all": times["ms_head"],
                  "replaced_ms": float(np.median(times["replaced"])), "replaced_ms_all": times["replaced"],
                  "ms_head_hbm_bytes": head_bytes, "replaced_hbm_bytes": old_bytes, "pred_agreement": agree}))
