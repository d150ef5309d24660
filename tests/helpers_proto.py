"""A numpy float64 restatement of the class-prototype contract in include/szn.h (szn_class_proto) and of utils.blend_prototypes, for the
tests, built from the single-view pieces of tests/helpers_msinfer.py (up_crop, view_sims, bound).  Also the adaptation cases the CPU and
the GPU tests share."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers_calib as HC  # noqa: E402
import helpers_msinfer as HM  # noqa: E402

EPS = 2.0 ** -52


# ---- the per-pixel restatement ---------------------------------------------------------------------------------------------------
def pixel_vectors(coarse, S, H, W, crop=None):
    """-> (s (B,H,W,E) float64: the upsampled, cropped score; sn (B,H,W): |s|; kappa (B,H,W): (sum_t w_t |C_t|) / |s|)"""
    crop = HM.CROP[S] if crop is None else crop
    s = HM.up_crop(coarse, S, H, W, crop)
    cn = np.linalg.norm(np.asarray(coarse, dtype=np.float64), axis=3, keepdims=True)
    wn = HM.up_crop(cn, S, H, W, crop)[..., 0]
    sn = np.linalg.norm(s, axis=3)
    with np.errstate(invalid="ignore", divide="ignore"):
        kappa = wn / sn
    return s, sn, kappa


def masks(labels, sn, K, classes, mode):
    """-> (part, contrib) (B,H,W) bool: the pixel participates (0 <= label < K, label in classes; None = all K) / contributes (UNIT:
    |s| finite and > 0; RAW: always)"""
    labels = np.asarray(labels)
    part = (labels >= 0) & (labels < K)
    if classes is not None:
        part &= np.isin(labels, list(classes))
    contrib = part & (np.isfinite(sn) & (sn > 0)) if mode == "unit" else part.copy()
    return part, contrib


def reference(S, H, W, coarse, labels, K, classes=None, mode="unit", crop=None):
    """-> dict: sums (K,E) float64, counts (K,2) int64, A (K,E): sum over the contributing pixels of sum_t |a w_t| |C_t,e| (a = 1 or
    1 / |s|), ubound (K,E): sum over the contributing pixels of helpers_msinfer.bound(1, kappa, E) (UNIT; zeros for RAW), npix (K,)"""
    coarse = np.asarray(coarse)
    E = coarse.shape[3]
    s, sn, kappa = pixel_vectors(coarse, S, H, W, crop)
    sabs = HM.up_crop(np.abs(coarse.astype(np.float64)), S, H, W, HM.CROP[S] if crop is None else crop)
    part, contrib = masks(labels, sn, K, classes, mode)
    sums, A, ub = np.zeros((K, E)), np.zeros((K, E)), np.zeros((K, E))
    counts = np.zeros((K, 2), dtype=np.int64)
    labels = np.asarray(labels)
    for k in np.unique(labels[part]):
        pk, ck = part & (labels == k), contrib & (labels == k)
        counts[k] = (pk.sum(), ck.sum())
        if mode == "unit":
            sums[k] = (s[ck] / sn[ck][:, None]).sum(axis=0)
            A[k] = (sabs[ck] / sn[ck][:, None]).sum(axis=0)
            ub[k] = HM.bound(1, kappa[ck], E).sum()
        else:
            sums[k] = s[ck].sum(axis=0)
            A[k] = sabs[ck].sum(axis=0)
    return dict(sums=sums, counts=counts, A=A, ubound=ub, npix=counts[:, 1].copy())


# ---- the coefficient-table form: sums[k][e] = sum_pos T[pos][k] coarse[pos][e] ----------------------------------------------------------
def tap_table(S, H, W, h, w, crop=None):
    """per pixel of one image: pos (H,W,4) int64, the linear position i * w + j of its four taps in tap order (I-1,J-1), (I-1,J), (I,J-1),
    (I,J) (-1: outside the map), and wt (H,W,4) float64, their weights (products of odd multiples of 1 / 2S: exact in fp32)"""
    crop = HM.CROP[S] if crop is None else crop
    Y, X = np.arange(H) + crop, np.arange(W) + crop
    I, ty, J, tx = Y // S, Y % S, X // S, X % S
    bil = lambda t: 1.0 - np.abs(t - (S - 0.5)) / S
    fy = np.stack([bil(ty + S), bil(ty)], axis=1)            # [:, 0]: vertex I - 1, [:, 1]: vertex I
    fx = np.stack([bil(tx + S), bil(tx)], axis=1)
    pos = np.empty((H, W, 4), dtype=np.int64)
    wt = np.empty((H, W, 4))
    for t in range(4):
        i, j = (I - 1 + (t >> 1))[:, None], (J - 1 + (t & 1))[None, :]
        ok = (i >= 0) & (i < h) & (j >= 0) & (j < w)
        pos[:, :, t] = np.where(ok, i * w + j, -1)
        wt[:, :, t] = fy[:, t >> 1][:, None] * fx[:, t & 1][None, :]
    assert (wt.astype(np.float32) == wt).all()
    return pos, wt


def coefficient_table(S, H, W, h, w, labels, coef, contrib, K):
    """T (B h w, K) float64: T[pos][k] = sum over the contributing pixels labelled k that blend pos of coef * w_t (coef (B,H,W): 1 for RAW,
    1 / |s| for UNIT)"""
    B = labels.shape[0]
    pos, wt = tap_table(S, H, W, h, w)
    T = np.zeros((B * h * w, K))
    for b in range(B):
        m = contrib[b]
        for t in range(4):
            ok = m & (pos[:, :, t] >= 0)
            np.add.at(T, (b * h * w + pos[:, :, t][ok], labels[b][ok]), wt[:, :, t][ok] * coef[b][ok])
    return T


def raw_reference_exact(S, H, W, coarse, labels, K, classes=None):
    """the RAW sums through the table form in extended precision: T and every product T * c are exact in float64 (12-bit weights summed
    over at most 4 S^2 pixels times 24-bit values), and the sum over the positions runs in long double -> (sums (K,E) float64: the exact
    sum rounded at most twice, T)"""
    coarse = np.asarray(coarse)
    B, h, w, E = coarse.shape
    labels = np.asarray(labels)
    part, contrib = masks(labels, np.ones(labels.shape), K, classes, "raw")
    T = coefficient_table(S, H, W, h, w, labels, np.ones(labels.shape), contrib, K)
    c = coarse.reshape(B * h * w, E).astype(np.longdouble)
    sums = np.zeros((K, E), dtype=np.longdouble)
    for k in np.flatnonzero(np.abs(T).sum(axis=0) > 0):
        nz = np.flatnonzero(T[:, k])
        sums[k] = (T[nz, k].astype(np.longdouble)[:, None] * c[nz]).sum(axis=0)
    return sums.astype(np.float64), T


def n_add(npix, npos):
    """the longest chain of rounded additions behind one element of the kernel's RAW sums: the products and the coefficients are exact, at
    most min(4 npix, npos) positions carry a non-zero coefficient (adding an exact zero does not round), the four waves of a block and
    the chunks meet in 2 + (chunks - 1) more additions, which the position count covers except for tiny maps (+ 4), and the reference
    itself is rounded once more (+ 1)"""
    return np.minimum(4 * np.asarray(npix), npos) + 5


def raw_bound(ref, npos):
    """|sums - ref| allowed for the RAW sums: n_add * 2^-52 * A"""
    return n_add(ref["npix"], npos)[:, None] * EPS * ref["A"]


def unit_bound(ref, npos):
    """|sums - ref| allowed for the UNIT sums: per contributing pixel helpers_msinfer.bound(1, kappa, E) -- a unit vector's component is
    the cosine against a basis vector and takes no more roundings than the similarity that bound was derived for -- plus the RAW term"""
    return ref["ubound"] + raw_bound(ref, npos)


# ---- utils.blend_prototypes restated --------------------------------------------------------------------------------------------------
def blend(emb, sums, counts, classes, alpha, min_pixels=1):
    """-> (K,E) float32: rows k of `classes` with counts[k][1] >= min_pixels, |sums[k]| != 0 and |e_k| != 0 become |e_k| d / |d|,
    d = (1 - alpha) e_k / |e_k| + alpha sums[k] / |sums[k]| (float64), unless d = 0; every other row, and every row at alpha = 0, is the
    input's"""
    out = np.array(emb, dtype=np.float32)
    if alpha == 0:
        return out
    for k in classes:
        e, p = out[k].astype(np.float64), np.asarray(sums[k], dtype=np.float64)
        en, pn = np.linalg.norm(e), np.linalg.norm(p)
        if counts[k][1] < min_pixels or not pn > 0 or not en > 0:
            continue
        d = (1 - alpha) * e / en + alpha * p / pn
        dn = np.linalg.norm(d)
        if dn > 0:
            out[k] = (en * d / dn).astype(np.float32)
    return out


# ---- the adaptation cases ----------------------------------------------------------------------------------------------------------------
#        name: (stride, E, K, H, W): the smallest shapes at which all six palette classes land inside the cropped window at both strides
ADAPT = {
    "a1_s32_e20_k33": (32, 20, 33, 70, 90),
    "a2_s8_e20_k33": (8, 20, 33, 33, 47),
    "a3_s32_e300_k59": (32, 300, 59, 70, 90),
    "a4_s8_e300_k59": (8, 300, 59, 33, 47),
}
ADAPT_NAMES = sorted(ADAPT)
ADAPT_B = 2
PAL = (0, 2, 1, 5, 3, 8)                # three seen classes and the three unseen classes 2, 5, 8 of unseen = range(2, K, 3), interleaved
ACC_BEFORE_MAX, ACC_AFTER_MIN = 0.25, 0.6       # conditions on the inputs (unseen-class pixel accuracy with the word vectors / adapted)
UNCLEAR_CAP = 0.05                      # share of the query pixels whose top-two margin may lie within twice the bound


def visual_directions(emb, unseen):
    """the direction the network is made to give each class's pixels: the word vector for a seen class, for an unseen class u a
    direction that is not its word vector, vis[u] = -roll(emb[u], E // 2)"""
    vis = np.array(emb, dtype=np.float32)
    E = vis.shape[1]
    for u in unseen:
        vis[u] = -np.roll(emb[u], E // 2)
    return vis


@functools.lru_cache(maxsize=None)
def adapt_case(name, which):
    """helpers_calib.case with three differences: the coarse classes are tiled from the palette, cls[b,i,j] = PAL[(i + 2j + b) % 6]; a
    pixel's label is the class of its heaviest tap (argmax of the upsampled one-hot map); the unseen classes' coarse vectors are drawn
    around visual_directions.  which = "support" | "query": two seeds (scale and noise differ).  Cached: treat as read-only."""
    S, E, K, H, W = ADAPT[name]
    B = ADAPT_B
    seed = 9000 + 10 * ADAPT_NAMES.index(name) + {"support": 1, "query": 2}[which]
    rng = np.random.RandomState(seed)
    emb = HC.embeddings(E, K)
    unseen = sorted(range(2, K, 3))
    h, w = HM.coarse_size(H, S), HM.coarse_size(W, S)
    b, i, j = np.meshgrid(np.arange(B), np.arange(h), np.arange(w), indexing="ij")
    slot = (i + 2 * j + b) % 6
    cls = np.asarray(PAL)[slot]
    scale = 0.5 + rng.rand(B, h, w, 1)
    sigma = 0.6 * np.linalg.norm(emb.astype(np.float64), axis=1).mean() / np.sqrt(E)
    vis = visual_directions(emb, unseen)
    coarse = (vis[cls] * scale + sigma * rng.randn(B, h, w, E)).astype(np.float32)
    onehot = (slot[..., None] == np.arange(6)).astype(np.float32)
    labels = np.asarray(PAL)[HM.up_crop(onehot, S, H, W, HM.CROP[S]).argmax(axis=3)].astype(np.int64)
    adapted = [u for u in unseen if u in PAL]
    return dict(S=S, E=E, K=K, B=B, H=H, W=W, h=h, w=w, coarse=coarse, emb=emb, labels=labels, unseen=unseen, adapted=adapted)


def predict(S, H, W, coarse, emb):
    """nearest class embedding in float64 -> dict: pred (B,H,W), margin (the winner's lead over the second), bound (per similarity)"""
    sim, kappa = HM.view_sims(coarse, S, H, W, H, W, False, emb)
    pred = HM.first_argmax(sim)
    top2 = np.sort(sim, axis=-1)[..., -2:]
    return dict(pred=pred, margin=top2[..., 1] - top2[..., 0], bound=HM.bound(1, kappa, emb.shape[1]))


def class_accuracy(pred, labels, classes):
    """share of the pixels labelled with one of `classes` that the prediction gets right"""
    m = np.isin(labels, list(classes))
    return float((pred[m] == labels[m]).mean())


@functools.lru_cache(maxsize=None)
def adapt_reference(name, mode="unit", alpha=1.0):
    """the whole chain in float64 -> dict: proto (reference() on the support map, classes = the unseen set), emb_adapted, before / after
    (predict() on the query map with the word vectors / the adapted matrix), acc_before, acc_after (over the three adapted classes)"""
    sup, qry = adapt_case(name, "support"), adapt_case(name, "query")
    proto = reference(sup["S"], sup["H"], sup["W"], sup["coarse"], sup["labels"], sup["K"], sup["unseen"], mode)
    emb2 = blend(sup["emb"], proto["sums"], proto["counts"], sup["unseen"], alpha)
    before = predict(qry["S"], qry["H"], qry["W"], qry["coarse"], qry["emb"])
    after = predict(qry["S"], qry["H"], qry["W"], qry["coarse"], emb2)
    return dict(proto=proto, emb_adapted=emb2, before=before, after=after,
                acc_before=class_accuracy(before["pred"], qry["labels"], qry["adapted"]),
                acc_after=class_accuracy(after["pred"], qry["labels"], qry["adapted"]))
