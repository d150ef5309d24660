#!/usr/bin/env python
"""szn_conse_head (ConSE zero-shot inference for the softmax network, the seen-class penalty swept in one pass) at B = 8, 512 x 512,
E = 300, T = 10, K = 21 and K = 59, with 1 and 33 gammas, on synthetic logit maps of the sizes the backbones give (17 x 17 at stride
32, 74 x 74 at stride 8).  Per (K, stride):
  (f) the floor: szn_fused_ce_head, loss and channel argmax, as softmax_predict calls it -- what validation cost before ConSE
  (a) szn_conse_head alone: hist [G][K][K] and the prediction at gamma 0
  (v) a validation step with ConSE: (f) for the loss, then (a), as conse_predict issues them
  (m) the materialised route with ONE gamma: szn_bilinear_up_crop_fwd to the (B,K,H,W) score, then utils.conse_infer (torch ops: sort,
      softmax, scatter, two einsums over E, the group maxima); a sweep of G gammas would repeat it G times
HIP events around N calls after warm-up, the variants alternating over R rounds; one JSON line with the medians.
Every buffer of (f), (a), (v) is allocated before the window; (a) rebuilds G = embed embed^T in every call (conse_prep_kernel), clears its
crossing tables and runs calib_hist_kernel; (m) allocates its intermediates inside torch.  The logits are 3 N(0,1) per coarse position; the
labels are 16 x 16 blocks of one class.  --quick: fewer calls (a smoke run of the tool itself)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zeroshotsemanticsegmentation_amd import _lib as L, heads, utils

QUICK = "--quick" in sys.argv[1:]
B, H, W, E, T = 8, 512, 512, 300, 10
R, N, N_MAT = (2, 5, 1) if QUICK else (5, 50, 3)
dev = torch.device("cuda")
gen = torch.Generator(device="cuda"); gen.manual_seed(1)
lib = L.load()
FP = C.POINTER(C.c_float)


def coarse_size(n, stride):
    m = n + 198
    for _ in range(5):
        m = (m + 1) // 2
    m -= 6
    return m if stride == 32 else 4 * m + 6


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


out = {"shape": [B, H, W, E], "top_t": T, "calls_per_window": N, "calls_per_window_materialised": N_MAT, "rounds": R}
for K in (21, 59):
    unseen_list = list(range(2, K, 3))
    unseen = L.class_set(unseen_list)
    emb = torch.randn(K, E, device=dev, generator=gen)
    tgt = torch.randint(0, K, (B, H // 16, W // 16), device=dev, generator=gen).repeat_interleave(16, 1).repeat_interleave(16, 2)
    tgt[:, :8, :] = -1
    tgt = tgt.contiguous()
    for stride in (32, 8):
        h = w = coarse_size(H, stride)
        crop = heads._CROP[stride]
        cmap = (3.0 * torch.randn(B, h, w, K, device=dev, generator=gen)).contiguous()
        ws_f = torch.empty(lib.szn_fused_ce_head_workspace_bytes(stride, B, h, w, K), dtype=torch.uint8, device=dev)
        loss = torch.empty(1, device=dev)
        pred_f = torch.empty(B, H, W, dtype=torch.int64, device=dev)
        pred_a = torch.empty(B, H, W, dtype=torch.int64, device=dev)
        score = torch.empty(B, K, H, W, device=dev)

        def run_f():
            L.call("szn_fused_ce_head", stride, B, h, w, K, K, 0, H, W, crop, L.ptr(cmap), L.ptr(tgt), None, 0, L.ptr(loss), None,
                   L.ptr(pred_f), L.SZN_F32, None, L.ptr(ws_f), L.stream_ptr())

        def run_m():
            L.call("szn_bilinear_up_crop_fwd", stride, B, h, w, K, K, 0, H, W, crop, L.ptr(cmap), L.ptr(score), L.stream_ptr())
            return utils.conse_infer(score, emb, unseen_list, T, 0.0)

        res = {"map": [h, w]}
        for G in (1, 33):
            gammas = np.linspace(-0.5, 0.5, G).astype(np.float32) if G > 1 else np.zeros(1, dtype=np.float32)
            gp = gammas.ctypes.data_as(FP)
            g0 = int(np.flatnonzero(gammas == 0.0)[0])
            ws_a = torch.empty(lib.szn_conse_head_workspace_bytes(stride, B, h, w, E, K, G), dtype=torch.uint8, device=dev)
            hist = torch.zeros(G, K, K, dtype=torch.int64, device=dev)

            def run_a():
                L.call("szn_conse_head", stride, B, h, w, K, K, 0, H, W, crop, E, L.ptr(cmap), L.ptr(emb), L.ptr(tgt), unseen, T, 0, G, gp,
                       L.ptr(hist), g0, L.ptr(pred_a), L.ptr(ws_a), L.stream_ptr())

            def run_v():
                run_f()
                run_a()

            run_f(); run_a(); ref = run_m()                          # warm-up, and the two routes agree up to fp32 ties
            torch.cuda.synchronize()
            agree = float((ref == pred_a).double().mean())
            tf, ta, tv = [], [], []
            for _ in range(R):
                tf.append(timed(run_f, N))
                ta.append(timed(run_a, N))
                tv.append(timed(run_v, N))
            res["g%d" % G] = {"f_softmax_ms": float(np.median(tf)), "a_conse_ms": float(np.median(ta)), "v_step_ms": float(np.median(tv)),
                              "f_ms_all": tf, "a_ms_all": ta, "v_ms_all": tv, "kernel": L.prev_kernel(),
                              "agrees_with_materialised": agree, "share_predicted_unseen": float(torch.isin(
                                  pred_a, torch.tensor(unseen_list, device=dev)).double().mean())}
        tm = [timed(run_m, N_MAT) for _ in range(R)]
        res["m_materialised_one_gamma_ms"] = float(np.median(tm))
        res["m_ms_all"] = tm
        res["m_over_a_g1"] = res["m_materialised_one_gamma_ms"] / res["g1"]["a_conse_ms"]
        out["k%d_s%d" % (K, stride)] = res
print(json.dumps(out))
