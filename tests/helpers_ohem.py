"""A numpy restatement of the hard-pixel-mining contract in include/szn.h (szn_ohem_head), for the tests, on the synthetic cases of
tests/helpers_calib.py.  Stage 1 (the own-class cosine) in float64 from helpers_calib.case_reference(name)["sim"]; stages 2-3 (bins,
histogram, cut, counts, relabel) in exact integers from a given conf."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers_calib as HC  # noqa: E402

BINS = 1024                      # SZN_OHEM_BINS
DROP = -1                        # heads.OHEM_DROP_LABEL
KEEP = 250                       # permille
THRESH = 0.0
OFF = -2.0                       # a threshold that is turned off (<= -1)
NAMES = HC.NAMES


def evaluated(tgt, K, skip=()):
    """the pixels pass 1 evaluates: 0 <= target < K and the label not in `skip`"""
    tgt = np.asarray(tgt)
    return (tgt >= 0) & (tgt < K) & ~np.isin(tgt, list(skip))


@functools.lru_cache(maxsize=None)
def case_cosine(name):
    """stage 1 in float64: (B,H,W) the cosine of every evaluated pixel of the case to its own class embedding, NaN elsewhere"""
    c, ref = HC.case(name), HC.case_reference(name)
    ev = evaluated(c["target"], c["K"])
    own = np.take_along_axis(ref["sim"], np.where(ev, c["target"], 0)[..., None], axis=-1)[..., 0]
    out = np.where(ev, own, np.nan)
    out.setflags(write=False)
    return out


def bins(conf):
    """q = 0 where c is NaN, else clamp(floor(c * 512 + 512), 0, 1023) in float32: c * 512 is exact, so this is the kernel's fmaf bit for
    bit"""
    c = np.asarray(conf, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        q = np.clip(np.floor(c * np.float32(512) + np.float32(512)), 0, BINS - 1)
    return np.where(np.isnan(c), 0, q).astype(np.int64)


def thresh_bin(thresh):
    """tbin = clamp(floor(thresh * 512 + 512), 0, 1024) in float32"""
    with np.errstate(over="ignore"):
        return int(np.clip(np.floor(np.float32(thresh) * np.float32(512) + np.float32(512)), 0, BINS))


def select(conf, tgt, K, keep_permille, thresh, skip=(), drop_label=DROP):
    """stages 2-3 in exact integers from conf (B,H,W; only its values on the evaluated pixels are read) -> dict qhist (B,BINS),
    n, keep, tmin, cut (B,), counts (B,2), target_out, dropped"""
    tgt = np.asarray(tgt)
    B = tgt.shape[0]
    ev = evaluated(tgt, K, skip)
    q = np.where(ev, bins(conf), 0)
    qhist = np.zeros((B, BINS), dtype=np.int64)
    for b in range(B):
        qhist[b] = np.bincount(q[b][ev[b]], minlength=BINS)
    n = qhist.sum(axis=1)
    keep = (n * keep_permille + 999) // 1000
    prefix = np.concatenate([np.zeros((B, 1), dtype=np.int64), qhist.cumsum(axis=1)], axis=1)       # prefix[b][t] = sum_{q < t}
    tbin = thresh_bin(thresh)
    tmin = np.zeros(B, dtype=np.int64)
    cut = np.zeros(B, dtype=np.int64)
    counts = np.zeros((B, 2), dtype=np.int64)
    for b in np.flatnonzero(n > 0):
        tmin[b] = 1 + np.flatnonzero(prefix[b, 1:] >= keep[b]).min()
        cut[b] = max(tmin[b], tbin)
        counts[b] = (n[b], prefix[b, cut[b]])
    dropped = ev & (q >= cut.reshape(B, 1, 1))
    out = np.array(tgt, dtype=np.int64, copy=True)
    out[dropped] = drop_label
    return dict(qhist=qhist, n=n, keep=keep, tmin=tmin, cut=cut, counts=counts, target_out=out, dropped=dropped, prefix=prefix)
