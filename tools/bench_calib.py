#!/usr/bin/env python
"""szn_calib_head (calibrated stacking: the seen-class penalty swept over 33 gammas in one pass) at B = 8, 512 x 512, E = 300, K = 59, on
synthetic coarse maps of the sizes the backbones give (17 x 17 at stride 32, 74 x 74 at stride 8), against what ONE uncalibrated
evaluation costs with the entry points that were there before it:
  (a) szn_fused_head_prepared, prediction only, + szn_confusion_hist_k (all / seen / unseen rows, as Trainer.validate calls it)
  (b) szn_calib_head filling hist [33][K][K] (no prediction stored)
HIP events around N calls after warm-up, the two alternating over R rounds; one JSON line with the medians and b / a per stride
(DESIGN.md section 7j).  What the times include: every buffer is allocated before the window; (a) reuses prepared embedding tables,
(b) rebuilds them in every call (fh_prep_kernel), clears its crossing tables (hipMemsetAsync) and runs calib_hist_kernel.
The maps hold a class embedding per coarse position, scaled by 0.5 + U[0,1) plus noise, so neighbouring pixels mostly agree on their best
seen and unseen class as they do on a trained network's map; the labels are 16 x 16 blocks of one class ("blocks", the headline) or
independent per pixel ("noise": the most distinct (label, class, class, bin) keys a wave can hold, so the most atomics)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zeroshotsemanticsegmentation_amd import _lib as L, heads

B, H, W, E, K, G, R, N = 8, 512, 512, 300, 59, 33, 5, 100
UNSEEN = list(range(2, K, 3))
GAMMAS = np.linspace(-0.5, 0.5, G).astype(np.float32)
dev = torch.device("cuda")
gen = torch.Generator(device="cuda"); gen.manual_seed(1)
lib = L.load()


def coarse_size(n, stride):
    m = n + 198
    for _ in range(5):
        m = (m + 1) // 2
    m -= 6
    return m if stride == 32 else 4 * m + 6


emb = torch.randn(K, E, device=dev, generator=gen)
blocks = torch.randint(0, K, (B, H // 16, W // 16), device=dev, generator=gen).repeat_interleave(16, 1).repeat_interleave(16, 2)
blocks[:, :8, :] = -1
LABELS = {"blocks": blocks.contiguous(), "noise": torch.randint(0, K, (B, H, W), device=dev, generator=gen)}
unseen = L.class_set(UNSEEN)
gp = GAMMAS.ctypes.data_as(C.POINTER(C.c_float))


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


out = {"shape": [B, H, W, E, K], "gammas": G, "calls_per_window": N, "rounds": R}
for stride in (32, 8):
    h = w = coarse_size(H, stride)
    cls = torch.randint(0, K, (B, h, w), device=dev, generator=gen)
    cmap = (emb[cls] * (0.5 + torch.rand(B, h, w, 1, device=dev, generator=gen))
            + 0.6 * emb.norm(dim=1).mean() / E ** 0.5 * torch.randn(B, h, w, E, device=dev, generator=gen)).contiguous()
    crop = heads._CROP[stride]
    ws_a = torch.empty(lib.szn_fused_head_workspace_bytes(B, h, w, E, K), dtype=torch.uint8, device=dev)
    L.call("szn_fused_head_prepare", E, K, L.ptr(emb), L.ptr(ws_a), L.stream_ptr())
    ws_b = torch.empty(lib.szn_calib_head_workspace_bytes(stride, B, h, w, E, K, G), dtype=torch.uint8, device=dev)
    pred = torch.empty(B, H, W, dtype=torch.int64, device=dev)
    hist_a = torch.zeros(3, K, K, dtype=torch.int64, device=dev)
    hist_b = torch.zeros(G, K, K, dtype=torch.int64, device=dev)
    for kind, tgt in LABELS.items():
        def run_a():
            L.call("szn_fused_head_prepared", stride, B, h, w, E, E, 0, H, W, crop, K, L.ptr(cmap), L.ptr(emb), None, None, None,
                   L.ptr(pred), L.SZN_F32, None, L.ptr(ws_a), L.stream_ptr())
            L.call("szn_confusion_hist_k", B * H * W, K, L.ptr(tgt), L.ptr(pred), unseen, L.ptr(hist_a), L.stream_ptr())

        def run_b():
            L.call("szn_calib_head", stride, B, h, w, E, E, 0, H, W, crop, K, L.ptr(cmap), L.ptr(emb), L.ptr(tgt), unseen, G, gp,
                   L.ptr(hist_b), -1, None, L.ptr(ws_b), L.stream_ptr())

        hist_a.zero_(); hist_b.zero_()
        run_a(); run_b()                                     # warm-up, and the two agree at gamma = 0
        torch.cuda.synchronize()
        same = bool(torch.equal(hist_a[0], hist_b[G // 2]))
        ta, tb = [], []
        for _ in range(R):
            ta.append(timed(run_a, N))
            tb.append(timed(run_b, N))
        a_ms, b_ms = float(np.median(ta)), float(np.median(tb))
        out["s%d_%s" % (stride, kind)] = {"map": [h, w], "a_plain_ms": a_ms, "b_calib_ms": b_ms, "b_over_a": b_ms / a_ms, "a_ms_all": ta,
                                          "b_ms_all": tb, "gamma0_hist_equals_plain": same}
print(json.dumps(out))
