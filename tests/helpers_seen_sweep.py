"""A numpy restatement of the seen-mask threshold contract in include/szn.h (szn_seenmask_margin, szn_seen_sweep_head), for the tests:
the margin in float64 and in float32 with the kernel's fmaf order, the grouped class rule built from the single-view pieces of
tests/helpers_msinfer.py (view_sims with the identity view, group_pred, margin), the per-tau histograms.  Also the synthetic cases the
CPU and the GPU tests share."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers_calib as HC  # noqa: E402
import helpers_msinfer as HM  # noqa: E402

CROP = 19
NEAR_TIE = 1e-5             # the project's usual rule: class assignment is compared where the top-2 cosine lead in the group exceeds it


# ---- the margin --------------------------------------------------------------------------------------------------------------------
def _taps(sm, H, W, crop=CROP):
    """the 8 (coarse value, filter tap index) pairs of every pixel in the kernel's order -- ci outer, then di, then dj: c (8,B,H,W)
    float32 (exact zeros outside the map) and (ky, kx) (8,H,W) with the tap of channel pair (ci, co) at wt[ci, co, ky, kx]"""
    sm = np.asarray(sm, dtype=np.float32)
    B, h, w, _ = sm.shape
    Y, X = np.arange(H) + crop, np.arange(W) + crop
    out = []
    for ci in range(2):
        for di in range(2):
            for dj in range(2):
                i, j = (Y >> 5) - 1 + di, (X >> 5) - 1 + dj
                ok = ((i >= 0) & (i < h))[:, None] & ((j >= 0) & (j < w))[None, :]
                c = sm[:, np.clip(i, 0, h - 1)[:, None], np.clip(j, 0, w - 1)[None, :], ci]
                c = np.where(ok[None], c, np.float32(0))
                ky, kx = (Y & 31) + 32 - 32 * di, (X & 31) + 32 - 32 * dj
                out.append((ci, c, np.broadcast_to(ky[:, None], (H, W)), np.broadcast_to(kx[None, :], (H, W))))
    return out


def margin64(sm, wt, H, W, crop=CROP):
    """-> (s1 - s0 in float64 (B,H,W), sum over the 16 products |c * w| (B,H,W))"""
    wt = np.asarray(wt, dtype=np.float64)
    s = np.zeros((2,) + (np.asarray(sm).shape[0], H, W))
    mag = np.zeros(s.shape[1:])
    for ci, c, ky, kx in _taps(sm, H, W, crop):
        for co in range(2):
            p = c.astype(np.float64) * wt[ci, co][ky, kx]
            s[co] += p
            mag += np.abs(p)
    return s[1] - s[0], mag


def fma32(a, b, c):
    """round32(a * b + c) for float32 arrays, once: the product is exact in float64, the sum's float64 rounding error is recovered
    (TwoSum) and decides the case where the float64 sum lies exactly between two float32 values.  (Results in the float32 denormal
    range are not covered: the synthetic cases hold none but exact zeros.)"""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    tie = (s.view(np.int64) & 0x1FFFFFFF) == 0x10000000
    nudge = np.where(err > 0, np.inf, -np.inf)
    s = np.where(tie & (err != 0), np.nextafter(s, nudge), s)
    return s.astype(np.float32)


def margin32(sm, wt, H, W, crop=CROP):
    """the kernel's float32 margin: s0 and s1 by one fmaf per tap in the order ci, di, dj from 0, then one float32 subtraction"""
    wt = np.asarray(wt, dtype=np.float32)
    B = np.asarray(sm).shape[0]
    s = [np.zeros((B, H, W), np.float32), np.zeros((B, H, W), np.float32)]
    for ci, c, ky, kx in _taps(sm, H, W, crop):
        for co in range(2):
            s[co] = fma32(c, np.broadcast_to(wt[ci, co][ky, kx], c.shape), s[co])
    with np.errstate(invalid="ignore"):
        return s[1] - s[0]


# ---- the class rule and the histograms -------------------------------------------------------------------------------------------
def group_answers(sim, unseen):
    """sim (B,H,W,K) -> (A, Bc, lead_A, lead_B): the grouped head's answer for a pixel in the seen group and in the unseen group (a
    class outside the group competes with 0, the first index wins, all-NaN gives 0) and the winner's lead over the next candidate"""
    K = sim.shape[-1]
    is_unseen = np.zeros(K, dtype=bool)
    is_unseen[list(unseen)] = True
    ga = np.broadcast_to(~is_unseen, sim.shape)
    gb = np.broadcast_to(is_unseen, sim.shape)
    return HM.group_pred(sim, ga), HM.group_pred(sim, gb), HM.margin(sim, ga), HM.margin(sim, gb)


def predict(A, Bc, margin, taus):
    """(G,B,H,W): A where margin > tau (a NaN compares false), else Bc"""
    t = np.asarray(taus).reshape((-1,) + (1,) * margin.ndim)
    with np.errstate(invalid="ignore"):
        return np.where(margin[None] > t, A[None], Bc[None]).astype(np.int64)


def bins(margin, taus):
    """the first g with not (margin > taus[g]); len(taus): never"""
    t = np.asarray(taus).reshape((-1,) + (1,) * margin.ndim)
    with np.errstate(invalid="ignore"):
        seen = margin[None] > t
    assert (seen[:-1] >= seen[1:]).all()                       # ascending taus: a prefix
    return seen.sum(axis=0)


histograms = HC.histograms                                     # (G,K,K): hist[g][t][pred_g] over the pixels with 0 <= t < K


def crossing_histograms(target, A, Bc, margin, taus, K):
    """the same histograms through the crossing tables XA[t][A][bin], XB[t][Bc][bin]"""
    G = len(taus)
    b = bins(margin, taus)
    ok = (target >= 0) & (target < K)
    XA = np.zeros((K, K, G + 1), dtype=np.int64)
    XB = np.zeros((K, K, G + 1), dtype=np.int64)
    np.add.at(XA, (target[ok], A[ok], b[ok]), 1)
    np.add.at(XB, (target[ok], Bc[ok], b[ok]), 1)
    out = np.zeros((G, K, K), dtype=np.int64)
    for g in range(G):
        out[g] = XA[:, :, g + 1:].sum(axis=2) + XB[:, :, :g + 1].sum(axis=2)
    return out


# ---- the synthetic cases ---------------------------------------------------------------------------------------------------------
#        name: (stride, E, K, H, W, B, seed)
CASES = {
    "s32_e20_k21": (32, 20, 21, 70, 100, 2, 201),
    "s32_e300_k59": (32, 300, 59, 33, 47, 2, 202),
    "s8_e20_k21": (8, 20, 21, 33, 47, 2, 203),
    "s8_e300_k59": (8, 300, 59, 70, 100, 1, 204),
}
NAMES = sorted(CASES)
UNSEEN_KINDS = ("zero", "high", "half", "most")


def unseen_sets(K):
    """{0}: the first out-of-group index flips between the groups; one high class; about half of the classes; all but two (a pixel
    with a negative cosine to both seen classes answers with an out-of-group index in the seen group)"""
    return {"zero": [0], "high": [K - 1], "half": list(range(1, K, 2)), "most": [k for k in range(K) if k not in (3, 7)]}


def embeddings(E, K):
    """K rows of width E: the first half are context rows of tests/golden, the second half their negation -- the word vectors all
    point roughly the same way, so a pixel near a negated row has a negative cosine to every row of the first half"""
    rows = np.load(os.path.join(HM.GOLDEN, "embeddings_context_%d.npy" % E)).astype(np.float32)
    n = (K + 1) // 2
    assert n <= rows.shape[0]
    return np.ascontiguousarray(np.concatenate([rows[:n], -rows[:n]], axis=0)[:K])


@functools.lru_cache(maxsize=None)
def case(name):
    """the class map of helpers_calib.case (a class embedding per position, scaled, plus noise) on the h x w map the backbone gives at
    the stride, with an all-zero corner (zero-norm pixels); a 2-channel 1/32 seen-mask map and a (2,2,64,64) filter bank; labels with
    -1, -2 and >= K regions.  Cached: treat as read-only."""
    S, E, K, H, W, B, seed = CASES[name]
    rng = np.random.RandomState(seed)
    emb = embeddings(E, K)
    h, w = HM.coarse_size(H, S), HM.coarse_size(W, S)
    cls = rng.randint(0, K, (B, h, w))
    scale = 0.5 + rng.rand(B, h, w, 1)
    sigma = 0.6 * np.linalg.norm(emb.astype(np.float64), axis=1).mean() / np.sqrt(E)
    fmap = (emb[cls] * scale + sigma * rng.randn(B, h, w, E)).astype(np.float32)
    n = 1 if S == 32 else 5
    fmap[:, :n, :n] = 0.0
    h32, w32 = HM.coarse_size(H, 32), HM.coarse_size(W, 32)
    sm = rng.randn(B, h32, w32, 2).astype(np.float32)
    wt = (0.1 * rng.randn(2, 2, 64, 64)).astype(np.float32)
    target = rng.randint(0, K, (B, H, W)).astype(np.int64)
    target[:, :3, :5] = -1
    target[:, -2:, :] = -2
    target[:, 10:12, 7:30] = K
    target[:, 12, 7:30] = K + 200
    return dict(S=S, E=E, K=K, B=B, H=H, W=W, h=h, w=w, h32=h32, w32=w32, fmap=fmap, emb=emb, sm=sm, wt=wt, target=target)


def taus_from(margin, n):
    """n ascending float32 thresholds for a margin map: for n >= 3 one below every margin, n - 2 of the map's own values (so that
    margin == tau occurs), one above every margin; for n < 3 the map's own values only"""
    vals = np.unique(np.asarray(margin, dtype=np.float32))
    vals = vals[np.isfinite(vals)]
    inner = n - 2 if n >= 3 else n
    pick = vals[np.linspace(0, vals.size - 1, inner + 2).astype(np.int64)[1:-1]]
    assert np.unique(pick).size == inner
    if n < 3:
        return pick.astype(np.float32)
    return np.concatenate([[vals[0] - np.float32(1)], pick, [vals[-1] + np.float32(1)]]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """-> dict: sim (B,H,W,K) float64, m32 (the kernel's float32 margin), per unseen kind (A, Bc, unclear (B,H,W) bool): a pixel is
    unclear when its lead in either group is below NEAR_TIE; a zero-norm pixel (dead: every similarity NaN) is clear, class 0"""
    c = case(name)
    sim, _ = HM.view_sims(c["fmap"], c["S"], c["H"], c["W"], c["H"], c["W"], False, c["emb"])
    dead = np.isnan(sim).all(axis=-1)
    out = dict(sim=sim, dead=dead, m32=margin32(c["sm"], c["wt"], c["H"], c["W"]))
    for kind, unseen in unseen_sets(c["K"]).items():
        A, Bc, la, lb = group_answers(sim, unseen)
        out[kind] = (A, Bc, ~dead & ~((la > NEAR_TIE) & (lb > NEAR_TIE)))
    return out
