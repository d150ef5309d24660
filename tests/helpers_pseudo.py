"""A numpy restatement of the pseudo-label contract in include/szn.h (szn_pseudo_head), for the tests, on the synthetic cases of
tests/helpers_calib.py.  Stage 1 (the candidate rule) in float64 on helpers_calib.reference; stages 2-3 (histogram, thresholds,
relabel) in exact integers from a given (cand, conf)."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers_calib as HC  # noqa: E402

HIDDEN = -3                      # datasets.HIDDEN_LABEL
BINS = 1024                      # SZN_PSEUDO_BINS
GAMMAS = (0.0, 0.125)            # both among helpers_calib.GAMMAS, so case_reference's `unclear` covers them
CONF_FLOOR = 0.2
KEEP = 300                       # permille
NAMES = HC.NAMES


@functools.lru_cache(maxsize=None)
def target(name):
    """the case's target with every unseen-labelled pixel hidden; the helper's -1 and -2 regions stay.  Cached: read-only."""
    c = HC.case(name)
    t = c["target"].copy()
    t[np.isin(t, c["unseen"])] = HIDDEN
    t.setflags(write=False)
    return t


def candidates(ref, tgt, gamma, conf_floor, unclear_at_gamma, cand_label=HIDDEN):
    """stage 1 in float64 -> (cand (B,H,W) int64, -1 = none; vb float64; unclear bool).  A pixel is a candidate when its target is
    cand_label, m is not NaN, NOT (m > gamma or (m == gamma and a < b)), and vb >= conf_floor.  Unclear: helpers_calib says so at this
    gamma, or |vb - conf_floor| <= 2 bound (fp32 may legitimately land on the other side of the floor)."""
    a, b, m = ref["a"], ref["b"], ref["m"]
    vb = np.take_along_axis(ref["sim"], b[..., None], axis=-1)[..., 0]
    with np.errstate(invalid="ignore"):
        takes_a = (m > gamma) | ((m == gamma) & (a < b))
        is_cand = (tgt == cand_label) & ~np.isnan(m) & ~takes_a & (vb >= conf_floor)
        unclear = unclear_at_gamma | ~(np.abs(vb - conf_floor) > 2 * ref["bound"])
    return np.where(is_cand, b, -1).astype(np.int64), vb, unclear


@functools.lru_cache(maxsize=None)
def case_candidates(name, gamma):
    ref = HC.case_reference(name)
    gi = int(np.flatnonzero(HC.GAMMAS == np.float32(gamma))[0])
    return candidates(ref, target(name), float(gamma), CONF_FLOOR, ref["unclear"][gi])


def bins(conf):
    """q = clamp(floor(c * 512 + 512), 0, 1023) in float32: c * 512 is exact, so this is the kernel's fmaf bit for bit"""
    c = np.asarray(conf, dtype=np.float32)
    return np.clip(np.floor(c * np.float32(512) + np.float32(512)), 0, BINS - 1).astype(np.int64)


def select(cand, conf, tgt, K, keep_permille):
    """stages 2-3 in exact integers from (cand, conf) -> dict qhist (K,BINS), thr (K,), counts (K,2), keep (K,), target_out"""
    is_cand = cand >= 0
    q = np.zeros(cand.shape, dtype=np.int64)
    q[is_cand] = bins(conf[is_cand])
    qhist = np.zeros((K, BINS), dtype=np.int64)
    np.add.at(qhist, (cand[is_cand], q[is_cand]), 1)
    n = qhist.sum(axis=1)
    keep = (n * keep_permille + 999) // 1000
    suffix = np.concatenate([qhist[:, ::-1].cumsum(axis=1)[:, ::-1], np.zeros((K, 1), dtype=np.int64)], axis=1)     # suffix[k][t], t <= BINS
    thr = np.full(K, BINS, dtype=np.int64)
    counts = np.zeros((K, 2), dtype=np.int64)
    for k in np.flatnonzero(n > 0):
        thr[k] = np.flatnonzero(suffix[k] >= keep[k]).max()
        counts[k] = (n[k], suffix[k, thr[k]])
    out = np.array(tgt, dtype=np.int64, copy=True)
    sel = is_cand.copy()
    sel[is_cand] = q[is_cand] >= thr[cand[is_cand]]
    out[sel] = cand[sel]
    return dict(qhist=qhist, thr=thr, counts=counts, keep=keep, target_out=out, selected=sel)
