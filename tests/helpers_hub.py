"""A numpy float64 restatement of the hubness-correction contract in include/szn.h (szn_hub_stats, szn_hub_head), for the tests, on the
cases and the similarities of tests/helpers_calib.py (imported, not edited)."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers_calib as HC  # noqa: E402
import helpers_msinfer as HM  # noqa: E402

PAD = -2                          # SZN_PAD_LABEL
BETA, MIN_SD = 1.0, 0.05          # the defaults (heads.HUB_BETA, heads.HUB_MIN_SD)
MODES = ("mean", "zscore")
# zscore on c2_s32_e300_k59: 0.19 of the pixels are unclear at some gamma with the float64 reference alone, 0.12 of them in-group near
# ties (E = 300 word vectors whose standardised similarities crowd together): the pair is left out of the prediction test
PRED_PAIRS = [(n, m) for m in MODES for n in HC.NAMES if (n, m) != ("c2_s32_e300_k59", "zscore")]


def gammas(mode):
    """helpers_calib.GAMMAS in mean mode, 4 x that in zscore mode (standardised similarities are a few units wide)"""
    return HC.GAMMAS if mode == "mean" else (4 * HC.GAMMAS).astype(np.float32)


def counted(sim, target=None):
    """(B,H,W) bool: the pixels the statistics see -- not padding, a finite norm > 0 (the float64 similarities are finite exactly there)"""
    ok = np.isfinite(sim).all(axis=-1)
    return ok if target is None else ok & (np.asarray(target) != PAD)


def moments(sim, ok):
    """-> n (B,) int64, mean (B,K), E[sim^2] (B,K) in float64 over the counted pixels (zeros where an image has none)"""
    n = ok.reshape(ok.shape[0], -1).sum(axis=1)
    s = np.where(ok[..., None], sim, 0.0)
    n1 = np.maximum(n, 1)[:, None]
    return n, s.sum(axis=(1, 2)) / n1, (s * s).sum(axis=(1, 2)) / n1


def table(n, mean, ex2, mode, beta=BETA, min_sd=MIN_SD):
    """(B,K,2) float64 (scale, shift) of include/szn.h from the moments; the identity row for an image without a counted pixel"""
    sd = np.sqrt(np.maximum(ex2 - mean * mean, 0.0))
    if mode == "mean":
        scale, shift = np.ones_like(mean), beta * mean
    else:
        f = np.maximum(sd, min_sd)
        scale, shift = 1.0 / f, beta * mean / f
    some = (n > 0)[:, None]
    return np.stack([np.where(some, scale, 1.0), np.where(some, shift, 0.0)], axis=-1)


def table_from_sums(sums, counts, mode, beta=BETA, min_sd=MIN_SD):
    """the finishing kernel's arithmetic in numpy doubles on the device's own int64 sums"""
    n = np.asarray(counts, dtype=np.float64)
    n1 = np.maximum(n, 1.0)[:, None]
    mean = sums[..., 0].astype(np.float64) / (n1 * 2.0 ** 20)
    ex2 = sums[..., 1].astype(np.float64) / (n1 * 2.0 ** 40)
    return table(np.asarray(counts), mean, ex2, mode, beta, min_sd)


def _group(adj, err, members):
    """(index, value, error of the best, unclear) of the first class of `members` holding the group's maximum of adj; unclear where the
    best's lead over some other class j of the group is <= 2 (e_best + e_j)"""
    members = np.asarray(members)
    sub, es = adj[..., members], err[..., members]
    idx = HM.first_argmax(sub)
    val = np.take_along_axis(sub, idx[..., None], axis=-1)[..., 0]
    eb = np.take_along_axis(es, idx[..., None], axis=-1)[..., 0]
    other = np.arange(len(members)) != idx[..., None]
    with np.errstate(invalid="ignore"):
        close = other & ~((val[..., None] - sub) > 2 * (eb[..., None] + es))
    return members[idx], val, eb, close.any(axis=-1)


def reference(sim, bound, unseen, tab, gam):
    """tab (B,K,2) (any float type; taken as exact) -> dict: adj (B,H,W,K) float64, a, b, m, pred (G,B,H,W), unclear (G,B,H,W).
    e_k = bound * scale_k + 4 * 2^-24 * |adj_k| per class; a pixel is unclear at gamma g when either group's best is within
    2 (e_best + e_j) of another class j of the group, or |m - g| <= 2 (e_a + e_b)."""
    K = sim.shape[-1]
    t = np.asarray(tab, dtype=np.float64)
    scale, shift = t[:, None, None, :, 0], t[:, None, None, :, 1]
    with np.errstate(invalid="ignore"):
        adj = sim * scale - shift
        err = bound[..., None] * np.abs(scale) + 4 * HM.U * np.abs(adj)
    is_unseen = np.zeros(K, dtype=bool)
    is_unseen[list(unseen)] = True
    a, va, ea, ca = _group(adj, err, np.flatnonzero(~is_unseen))
    b, vb, eb, cb = _group(adj, err, np.flatnonzero(is_unseen))
    g = np.asarray(gam, dtype=np.float64).reshape(-1, 1, 1, 1)
    with np.errstate(invalid="ignore"):
        m = va - vb
        unclear = (ca | cb)[None] | ~(np.abs(m[None] - g) > 2 * (ea + eb)[None])
    return dict(adj=adj, a=a, b=b, m=m, pred=HC.predict(a, b, m, gam), unclear=unclear)


@functools.lru_cache(maxsize=None)
def case_moments(name):
    """the float64 moments of case `name`: (counted (B,H,W), n, mean, E[sim^2])"""
    c, ref = HC.case(name), HC.case_reference(name)
    ok = counted(ref["sim"], c["target"])
    return (ok,) + moments(ref["sim"], ok)


def case_reference(name, mode, tab=None):
    """reference() of case `name` at gammas(mode), with the float64 table of the mode unless `tab` is given"""
    c, ref = HC.case(name), HC.case_reference(name)
    if tab is None:
        _, n, mean, ex2 = case_moments(name)
        tab = table(n, mean, ex2, mode)
    return reference(ref["sim"], ref["bound"], c["unseen"], tab, gammas(mode))


def skew(counts):
    """the skewness of a vector of counts, population moments"""
    x = np.asarray(counts, dtype=np.float64)
    d = x - x.mean()
    return float((d ** 3).mean() / (d * d).mean() ** 1.5)
