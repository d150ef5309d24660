"""numpy restatement of the visualisation contract (include/szn.h, "validation visualisations"): pixel recovery, grey, colour map, overlay,
mask, noise, both panel layouts and the mosaic.  Written from the contract, not from the kernel; integer-exact, so the GPU tests compare
with np.array_equal.  Nothing here touches a GPU.

Used by tests/test_viz_ref.py (CPU: ties the restatement to PIL, to the literal colours and to helpers_state's generator) and by
tests/test_gpu_viz.py (MI355X: the kernel, the wrappers and the trainers against it).
"""
import math

import numpy as np

MEAN_BGR = np.array([104.00698793, 116.66876762, 122.67891434], dtype=np.float64)
_M64 = (1 << 64) - 1


def transform(img_u8, mean_bgr=MEAN_BGR):
    """uint8 RGB (B,H,W,3) -> the network input, f32 (B,3,H,W) BGR minus mean (float64 subtraction, one rounding)"""
    return (img_u8[..., ::-1].astype(np.float64) - mean_bgr).astype(np.float32).transpose(0, 3, 1, 2).copy()


def recover(x_f32, mean_bgr=MEAN_BGR, rounding=True):
    """network input f32 (B,3,H,W) -> uint8 RGB (B,H,W,3): v = x + mean in float64, floor(v + 0.5) (or truncation), clamp, BGR -> RGB"""
    v = x_f32.astype(np.float64).transpose(0, 2, 3, 1) + mean_bgr
    u = np.floor(v + 0.5) if rounding else np.trunc(v)
    return np.clip(u, 0, 255).astype(np.uint8)[..., ::-1].copy()


def grey(rgb_u8):
    r, g, b = (rgb_u8[..., i].astype(np.int64) for i in range(3))
    return ((19595 * r + 38470 * g + 7471 * b + 32768) >> 16).astype(np.uint8)


def colormap(n=256):
    cmap = np.zeros((n, 3), dtype=np.uint8)
    for k in range(n):
        c = k
        for j in range(8):
            cmap[k, 0] |= (c & 1) << (7 - j)
            cmap[k, 1] |= ((c >> 1) & 1) << (7 - j)
            cmap[k, 2] |= ((c >> 2) & 1) << (7 - j)
            c >>= 3
    return cmap


def colour(lbl, K):
    """(…) labels -> (…,3) uint8; outside [0, K) is black"""
    valid = (lbl >= 0) & (lbl < K)
    return np.where(valid[..., None], colormap(256)[np.where(valid, lbl, 0)], 0).astype(np.uint8)


def overlay(col, g):
    return ((col.astype(np.int64) + g[..., None].astype(np.int64)) >> 1).astype(np.uint8)


def mask(lbl, K, unseen):
    seen = (lbl >= 0) & (lbl < K) & ~np.isin(lbl, list(unseen))
    return np.repeat((seen * 255).astype(np.uint8)[..., None], 3, axis=-1)


def splitmix64(z):
    """on Python integers (no numpy wrap-around involved)"""
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def noise_counters(B, H, W):
    """(B,H,W,3) Python-int counters 3 * ((b*H + y)*W + x) + c"""
    return (3 * np.arange(B * H * W, dtype=np.int64)[:, None] + np.arange(3)).reshape(B, H, W, 3)


def noise(B, H, W, seed):
    base = ((int(seed) & _M64) * 0xD1342543DE82EF95) & _M64
    out = np.zeros((B, H, W, 3), dtype=np.uint8)
    cnt = noise_counters(B, H, W)
    flat, oflat = cnt.reshape(-1), out.reshape(-1)
    for i in range(flat.size):
        h = splitmix64((base + int(flat[i])) & _M64)
        oflat[i] = ((h >> 40) * 255) >> 24
    return out


def as_rgb(img, mean_bgr=MEAN_BGR):
    """either image kind -> uint8 RGB (B,H,W,3)"""
    return img if img.dtype == np.uint8 else recover(img, mean_bgr)


def segmentation(img, lbl_true, lbl_pred, K, unseen=None, seed=1337, mean_bgr=MEAN_BGR):
    """-> (B, rows*H, n_col*W, 3) uint8"""
    rgb = as_rgb(img, mean_bgr)
    B, H, W, _ = rgb.shape
    g = grey(rgb)
    unl = None
    if lbl_true is not None:
        unl = (lbl_true < 0) | (lbl_true >= K)
        nz = noise(B, H, W, seed)
    rows = []
    for lbl in ([lbl_true] if lbl_true is not None else []) + [lbl_pred]:
        col = colour(lbl, K)
        panels = [rgb, col, overlay(col, g)] + ([mask(lbl, K, unseen)] if unseen else [])
        for p in panels[1:]:
            if unl is not None:
                p[unl] = nz[unl]
        rows.append(np.concatenate(panels, axis=2))
    return np.concatenate(rows, axis=1)


def seenmask(img, lbl_true, lbl_pred, seed=1337, mean_bgr=MEAN_BGR):
    """-> (B, H, 3W, 3) uint8: image | 255 * (lbl_true == 1) | 255 * (lbl_pred == 1), noise where lbl_true < 0"""
    rgb = as_rgb(img, mean_bgr)
    B, H, W, _ = rgb.shape
    unl = lbl_true < 0
    nz = noise(B, H, W, seed)
    panels = [rgb] + [np.repeat(((l == 1) * 255).astype(np.uint8)[..., None], 3, axis=-1) for l in (lbl_true, lbl_pred)]
    for p in panels[1:]:
        p[unl] = nz[unl]
    return np.concatenate(panels, axis=2)


def tile_shape(n):
    rows = max(math.isqrt(n), 1)
    return rows, -(-n // rows)


def mosaic(vizs):
    """list of (h,w,3) uint8 -> the mosaic: cells of the largest height / width, each picture centred on black, nothing resampled"""
    rows, cols = tile_shape(len(vizs))
    ch, cw = max(v.shape[0] for v in vizs), max(v.shape[1] for v in vizs)
    out = np.zeros((rows * ch, cols * cw, 3), dtype=np.uint8)
    for i, v in enumerate(vizs):
        y, x = (i // cols) * ch + (ch - v.shape[0]) // 2, (i % cols) * cw + (cw - v.shape[1]) // 2
        out[y:y + v.shape[0], x:x + v.shape[1]] = v
    return out
