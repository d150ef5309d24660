"""A numpy float64 restatement of the calibrated-stacking contract in include/szn.h (szn_calib_head), for the tests, built from the
single-view pieces of tests/helpers_msinfer.py (view_sims with the identity view, first_argmax, bound).  Also the synthetic cases the
CPU and the GPU tests share."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers_msinfer as HM  # noqa: E402

GAMMAS = np.linspace(-0.5, 0.5, 17).astype(np.float32)          # contains 0.0 exactly
assert GAMMAS[8] == 0.0

#        name: (stride, E, K, H, W, B, seed)
CASES = {
    "c1_s32_e5_k21": (32, 5, 21, 33, 47, 2, 101),
    "c2_s32_e300_k59": (32, 300, 59, 33, 47, 2, 102),
    "c3_s8_e20_k33": (8, 20, 33, 33, 47, 2, 103),
    "c4_s32_e20_k70": (32, 20, 70, 33, 47, 2, 104),
    "c5_s8_e300_k59": (8, 300, 59, 33, 47, 2, 105),
    "c6_s32_e20_k33_70x90": (32, 20, 33, 70, 90, 1, 106),
    "c7_s8_e5_k21_70x90": (8, 5, 21, 70, 90, 1, 107),
}
NAMES = sorted(CASES)


def embeddings(E, K):
    """K rows of width E: the context rows of tests/golden, then their negation, then the rows rolled by one channel.  (Not
    helpers_msinfer.embeddings: its context and pascal rows share words, which gives exactly tied classes across the two groups.)"""
    rows = np.load(os.path.join(HM.GOLDEN, "embeddings_context_%d.npy" % E)).astype(np.float32)
    full = np.concatenate([rows, -rows, np.roll(rows, 1, axis=1)], axis=0)
    assert K <= full.shape[0]
    return np.ascontiguousarray(full[:K])


@functools.lru_cache(maxsize=None)
def case(name):
    """a synthetic case: every coarse position holds a class embedding scaled by 0.5 + U[0,1) plus noise of 0.6 mean|e| / sqrt(E) per
    channel, on the h x w map the backbone gives for H x W; labels with -1 / -2 regions.  Cached: treat as read-only."""
    S, E, K, H, W, B, seed = CASES[name]
    rng = np.random.RandomState(seed)
    emb = embeddings(E, K)
    h, w = HM.coarse_size(H, S), HM.coarse_size(W, S)
    cls = rng.randint(0, K, (B, h, w))
    scale = 0.5 + rng.rand(B, h, w, 1)
    sigma = 0.6 * np.linalg.norm(emb.astype(np.float64), axis=1).mean() / np.sqrt(E)
    coarse = (emb[cls] * scale + sigma * rng.randn(B, h, w, E)).astype(np.float32)
    target = rng.randint(0, K, (B, H, W)).astype(np.int64)
    target[:, :3, :5] = -1
    target[:, -2:, :] = -2
    unseen = sorted(set(range(2, K, 3)) | ({K - 1} if K > 64 else set()))
    return dict(S=S, E=E, K=K, B=B, H=H, W=W, h=h, w=w, coarse=coarse, emb=emb, target=target, unseen=unseen, gammas=GAMMAS)


def group_best(sim, members):
    """(index, value, lead over the group's second) of the first class of `members` holding the group's maximum"""
    members = np.asarray(members)
    sub = sim[..., members]
    idx = HM.first_argmax(sub)
    val = np.take_along_axis(sub, idx[..., None], axis=-1)[..., 0]
    if len(members) > 1:
        rest = np.where(np.arange(len(members)) == idx[..., None], -np.inf, sub)
        with np.errstate(invalid="ignore"):
            lead = val - rest.max(axis=-1)
    else:
        lead = np.full(val.shape, np.inf)
    return members[idx], val, lead


def predict(a, b, m, gammas):
    """(G,B,H,W): 0 where m is NaN; a where m > gamma, or m == gamma and a < b; else b"""
    g = np.asarray(gammas).reshape((-1,) + (1,) * m.ndim)
    with np.errstate(invalid="ignore"):
        take_a = (m > g) | ((m == g) & (a < b))
    return np.where(np.isnan(m), 0, np.where(take_a, a, b)).astype(np.int64)


def histograms(target, pred, K):
    """(G,K,K): hist[g][t][pred_g] over the pixels with 0 <= t < K"""
    ok = (target >= 0) & (target < K)
    out = np.zeros((pred.shape[0], K, K), dtype=np.int64)
    for g in range(pred.shape[0]):
        out[g] = np.bincount(K * target[ok] + pred[g][ok], minlength=K * K).reshape(K, K)
    return out


def crossing_histograms(target, a, b, m, gammas, K):
    """the same histograms through the crossing tables: bin = the first g at which the pixel takes b (G: never), XA[t][a][bin],
    XB[t][b][bin]; hist[g][t][k] = sum_{bin > g} XA[t][k][bin] + sum_{bin <= g} XB[t][k][bin]"""
    G = len(gammas)
    nan = np.isnan(m)
    a, b = np.where(nan, 0, a), np.where(nan, 0, b)
    g = np.asarray(gammas).reshape((-1,) + (1,) * m.ndim)
    with np.errstate(invalid="ignore"):
        take_a = (m > g) | ((m == g) & (a < b))
    assert (take_a[:-1] >= take_a[1:]).all()                   # ascending gammas: a prefix
    bins = np.where(nan, G, take_a.sum(axis=0))
    ok = (target >= 0) & (target < K)
    XA = np.zeros((K, K, G + 1), dtype=np.int64)
    XB = np.zeros((K, K, G + 1), dtype=np.int64)
    np.add.at(XA, (target[ok], a[ok], bins[ok]), 1)
    np.add.at(XB, (target[ok], b[ok], bins[ok]), 1)
    out = np.zeros((G, K, K), dtype=np.int64)
    for gi in range(G):
        out[gi] = XA[:, :, gi + 1:].sum(axis=2) + XB[:, :, :gi + 1].sum(axis=2)
    return out


def reference(S, H, W, coarse, emb, unseen, gammas):
    """-> dict: sim (B,H,W,K) float64, a, b, m, pred (G,B,H,W), kappa, bound, unclear (G,B,H,W) bool.  A pixel is unclear at gamma g
    when its lead inside either group is <= 2 bound or |m - gamma_g| <= 4 bound: there fp32 may legitimately decide otherwise.
    bound = helpers_msinfer.bound(1, kappa, E) per similarity (twice that for the difference of two)."""
    K, E = emb.shape
    sim, kappa = HM.view_sims(coarse, S, H, W, H, W, False, emb)
    is_unseen = np.zeros(K, dtype=bool)
    is_unseen[list(unseen)] = True
    a, va, lead_a = group_best(sim, np.flatnonzero(~is_unseen))
    b, vb, lead_b = group_best(sim, np.flatnonzero(is_unseen))
    with np.errstate(invalid="ignore"):
        m = va - vb
    bound = HM.bound(1, kappa, E)
    g = np.asarray(gammas, dtype=np.float64).reshape(-1, 1, 1, 1)
    with np.errstate(invalid="ignore"):
        inside = ~((lead_a > 2 * bound) & (lead_b > 2 * bound))
        unclear = inside[None] | ~(np.abs(m[None] - g) > 4 * bound[None])
    return dict(sim=sim, a=a, b=b, m=m, pred=predict(a, b, m, gammas), kappa=kappa, bound=bound, unclear=unclear)


@functools.lru_cache(maxsize=None)
def case_reference(name):
    c = case(name)
    return reference(c["S"], c["H"], c["W"], c["coarse"], c["emb"], c["unseen"], c["gammas"])
