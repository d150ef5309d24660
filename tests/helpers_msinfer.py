"""A numpy float64 restatement of the multi-scale inference contract in include/szn.h (szn_resize_flip_f32, szn_ms_head), for the
tests.  The stride-S bilinear kernel comes from the oracle (get_upsampling_weight); the position map, the resize, the similarities,
the group rule and the first-index argmax are restated here.  Also the synthetic cases the CPU and the GPU tests share."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import szn_oracle as O  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CROP = {32: 19, 8: 31}
U = 2.0 ** -24            # unit roundoff of fp32


def axis_map(n_dst, n_src, flip=False):
    """the 16.16 pixel-centre map of one axis: destination 0..n_dst-1 (mirrored first when flip) -> (i0, i1, w) with the 11-bit
    weight w of i1"""
    g = np.arange(n_dst, dtype=np.int64)
    if flip:
        g = n_dst - 1 - g
    step = ((n_src << 16) + n_dst // 2) // n_dst
    s = (((2 * g + 1) * step) >> 1) - 32768
    s = np.clip(s, 0, (n_src - 1) << 16)
    i0 = s >> 16
    i1 = np.minimum(i0 + 1, n_src - 1)
    w = (s & 0xffff) >> 5
    return i0, i1, w


def resize_flip(x, Hs, Ws, flip=False):
    """szn_resize_flip_f32 on a (B,C,H,W) float32 array, in the contract's operation order -> float32 (bit-exact)"""
    B, C, H, W = x.shape
    y0, y1, wy = axis_map(Hs, H)
    # the view's pixel xo reads the position of xo' = Ws-1-xo
    x0, x1, wx = axis_map(Ws, W, flip)
    xd = x.astype(np.float64)
    wy = wy[:, None].astype(np.float64)
    wx = wx[None, :].astype(np.float64)
    p00, p01 = xd[:, :, y0][:, :, :, x0], xd[:, :, y0][:, :, :, x1]
    p10, p11 = xd[:, :, y1][:, :, :, x0], xd[:, :, y1][:, :, :, x1]
    top = (2048 - wx) * p00 + wx * p01
    bot = (2048 - wx) * p10 + wx * p11
    return (((2048 - wy) * top + wy * bot) / 4194304.0).astype(np.float32)


def up_crop(coarse, S, Hs, Ws, crop):
    """szn_bilinear_up_crop_fwd's definition in float64: coarse (B,h,w,E) -> (B,Hs,Ws,E)"""
    c = np.asarray(coarse, dtype=np.float64)
    B, h, w, E = c.shape
    w2 = O.get_upsampling_weight(1, 1, 2 * S)[0, 0].astype(np.float64)
    full = np.zeros((B, S * (h + 1), S * (w + 1), E))
    for ky in range(2 * S):
        for kx in range(2 * S):
            full[:, ky:ky + S * h:S, kx:kx + S * w:S] += w2[ky, kx] * c
    assert Hs + crop <= full.shape[1] and Ws + crop <= full.shape[2]
    return full[:, crop:crop + Hs, crop:crop + Ws]


def view_to_pixels(v, H, W, flip):
    """the 11-bit-weighted blend of a (B,Hs,Ws,E) view volume at the original pixels (B,H,W,E): xm = flip ? W-1-x : x"""
    Hs, Ws = v.shape[1:3]
    y0, y1, wy = axis_map(H, Hs)
    x0, x1, wx = axis_map(W, Ws, flip)
    wy = wy[None, :, None, None].astype(np.float64)
    wx = wx[None, None, :, None].astype(np.float64)
    top = (2048 - wx) * v[:, y0][:, :, x0] + wx * v[:, y0][:, :, x1]
    bot = (2048 - wx) * v[:, y1][:, :, x0] + wx * v[:, y1][:, :, x1]
    return ((2048 - wy) * top + wy * bot) / 4194304.0


def view_sims(coarse, S, H, W, Hs, Ws, flip, embed, crop=None):
    """-> (sim (B,H,W,K), kappa (B,H,W)) of one view: sim = s . e_k / (|s| * (|e_k| == 0 ? 1 : |e_k|)); kappa = (sum_p W_p |C_p|) / |s|,
    the sum over the coarse vectors the pixel blends with their composite weights (the blend of the norms: the weights are linear)"""
    crop = CROP[S] if crop is None else crop
    e = np.asarray(embed, dtype=np.float64)
    en = np.linalg.norm(e, axis=1)
    en = np.where(en == 0, 1.0, en)
    s = view_to_pixels(up_crop(coarse, S, Hs, Ws, crop), H, W, flip)
    cn = np.linalg.norm(np.asarray(coarse, dtype=np.float64), axis=3, keepdims=True)
    wn = view_to_pixels(up_crop(cn, S, Hs, Ws, crop), H, W, flip)[..., 0]
    sn = np.linalg.norm(s, axis=3)
    with np.errstate(invalid="ignore", divide="ignore"):
        sim = (s @ e.T) / (sn[..., None] * en)
        kappa = wn / sn
    return sim, kappa


def in_group(K, unseen, mode, gmap=None, target=None, shape=None):
    """(B,H,W,K) bool: class k competes with its own value at the pixel (group modes of szn_fused_head_grouped)"""
    if mode == 0:
        return np.ones(tuple(shape) + (K,), dtype=bool)
    is_unseen = np.zeros(K, dtype=bool)
    is_unseen[list(unseen or [])] = True
    take_unseen = (np.asarray(gmap) == 0) if mode == 1 else np.isin(np.asarray(target), list(unseen or []))
    return is_unseen[None, None, None, :] == take_unseen[..., None]


def first_argmax(vals):
    """the first k whose value exceeds the running best, starting from k = 0 (a NaN never exceeds and is never exceeded)"""
    best = np.zeros(vals.shape[:-1], dtype=np.int64)
    bv = vals[..., 0].copy()
    with np.errstate(invalid="ignore"):
        for k in range(1, vals.shape[-1]):
            gt = vals[..., k] > bv
            bv = np.where(gt, vals[..., k], bv)
            best = np.where(gt, k, best)
    return best


def group_pred(acc, grp):
    """the group rule: a class outside the pixel's group competes with 0"""
    return first_argmax(np.where(grp, acc, 0.0))


def margin(acc, grp, zero_rows=None):
    """winner's lead over the best other candidate.  The candidates that hold exactly 0 by construction -- the classes outside the
    group, and the classes whose embedding is all zero (zero_rows (K,) bool: s . 0 = 0 in any arithmetic) -- are ONE candidate: they
    tie exactly in the kernel as in the reference, and the first of them wins among them"""
    vals = np.where(grp, acc, 0.0)
    pred = first_argmax(vals)
    win = np.take_along_axis(vals, pred[..., None], axis=-1)[..., 0]
    K = vals.shape[-1]
    zero = ~grp if zero_rows is None else (~grp | np.asarray(zero_rows, dtype=bool))
    pred_zero = np.take_along_axis(zero, pred[..., None], axis=-1)[..., 0]
    other = np.ones(vals.shape, dtype=bool)
    other &= np.arange(K) != pred[..., None]
    other &= ~(pred_zero[..., None] & zero)
    with np.errstate(invalid="ignore"):
        second = np.where(other, vals, -np.inf).max(axis=-1)
        m = win - second
    return np.where(np.isnan(m), 0.0, m)


def reference(S, H, W, views, embed, unseen=None, mode=0, gmap=None, target=None, crop=None):
    """views: [(coarse (B,h,w,E) float32, Hs, Ws, flip)] -> dict: acc (B,H,W,K) float64 (the ungrouped sum over the views, in order),
    grp, pred (int64), kappa (max over the views), margin"""
    K = np.asarray(embed).shape[0]
    acc = kappa = None
    for coarse, Hs, Ws, flip in views:
        sim, kap = view_sims(coarse, S, H, W, Hs, Ws, flip, embed, crop)
        acc = sim if acc is None else acc + sim
        kappa = kap if kappa is None else np.fmax(kappa, kap)
    grp = in_group(K, unseen, mode, gmap, target, acc.shape[:3])
    zero_rows = ~np.asarray(embed).any(axis=1)
    return dict(acc=acc, grp=grp, pred=group_pred(acc, grp), kappa=kappa, margin=margin(acc, grp, zero_rows))


def bound(n_views, kappa, E):
    """|acc - reference| allowed per entry: V * 4 kappa^2 (E + 96) 2^-24 -- fp32 rounding of an E-term dot product, a <= 81-term Gram
    form and the weight products, Cauchy-Schwarz on the products, the norm's error half its square's"""
    return n_views * 4.0 * kappa ** 2 * (E + 96) * U


# ---- the backbone's map geometry ------------------------------------------------------------------------------------------------
def coarse_size(n, S):
    """rows (columns) of the map the head reads for an input of n rows: FCN32s' 1/32 map (conv1_1 pad 100, five ceil pools, the 7 x 7
    fc6) or FCN8s' 1/8 fused map (two x2 upsamplings, kernel 4, of it)"""
    m = n + 198
    for _ in range(5):
        m = (m + 1) // 2
    m -= 6
    return m if S == 32 else 4 * m + 6


def view_sizes(H, W, scales, flip):
    out = []
    for s in sorted(scales):
        size = (max(1, int(H * s + 0.5)), max(1, int(W * s + 0.5)))
        out += [size + (False,)] + ([size + (True,)] if flip else [])
    return out


def embeddings(E, K, zero_row=None):
    """K rows of width E from tests/golden/embeddings_*: the context rows, then the pascal rows, then negated context rows"""
    ctx = np.load(os.path.join(GOLDEN, "embeddings_context_%d.npy" % E))
    pas = np.load(os.path.join(GOLDEN, "embeddings_pascal_%d.npy" % E))
    rows = np.concatenate([ctx, pas, -ctx], axis=0)
    assert K <= rows.shape[0]
    emb = np.ascontiguousarray(rows[:K], dtype=np.float32)
    if zero_row is not None:
        emb[zero_row] = 0.0
    return emb


H0, W0 = 33, 47
SCALES = (0.5, 1.0, 1.5)
#       name: (stride, E, K, zero_row, seed)
CASES = {
    "s32_e5_k21": (32, 5, 21, 3, 101),
    "s32_e300_k59": (32, 300, 59, 7, 102),
    "s8_e20_k33": (8, 20, 33, None, 103),
    "s32_e20_k70": (32, 20, 70, 66, 104),
}


@functools.lru_cache(maxsize=None)
def case(name, B=2):
    """a synthetic case: per view a (B,h,w,E) map, uniform in [0.5, 1.5] (different per image), with the h x w the backbone gives for
    that view's size; embeddings; labels with -1 / -2 pixels; a group map; an unseen set.  Cached: treat as read-only."""
    S, E, K, zero_row, seed = CASES[name]
    rng = np.random.RandomState(seed)
    views = []
    for Hs, Ws, flip in view_sizes(H0, W0, SCALES, True):
        coarse = (rng.rand(B, coarse_size(Hs, S), coarse_size(Ws, S), E) + 0.5).astype(np.float32)
        views.append((coarse, Hs, Ws, flip))
    emb = embeddings(E, K, zero_row)
    target = rng.randint(0, K, (B, H0, W0)).astype(np.int64)
    target[:, :3, :5] = -1
    target[:, -2:, :] = -2
    gmap = rng.randint(0, 2, (B, H0, W0)).astype(np.int64)
    unseen = sorted(set(range(2, K, 3)) | ({K - 1} if K > 64 else set()))
    return dict(S=S, E=E, K=K, B=B, H=H0, W=W0, views=views, emb=emb, target=target, gmap=gmap, unseen=unseen)


@functools.lru_cache(maxsize=None)
def case_reference(name, mode):
    c = case(name)
    return reference(c["S"], c["H"], c["W"], c["views"], c["emb"], c["unseen"], mode, c["gmap"], c["target"])
