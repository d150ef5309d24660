"""CPU: the numpy restatement of szn_ohem_head (tests/helpers_ohem.py) keeps the contract's invariants on the shared synthetic cases, and
the fixed test parameters (keep 250 permille, thresh 0.0) reach both branches of cut = max(tmin, tbin): the threshold decides in c2, c4
and c5, the per-image budget in c1, c3, c6 and c7."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers_calib as HC  # noqa: E402
import helpers_ohem as HO  # noqa: E402

THRESHOLD_DRIVEN = ("c2_s32_e300_k59", "c4_s32_e20_k70", "c5_s8_e300_k59")


def _select(name, keep=HO.KEEP, thresh=HO.THRESH, **kw):
    c = HC.case(name)
    return c, HO.select(HO.case_cosine(name), c["target"], c["K"], keep, thresh, **kw)


@pytest.mark.parametrize("name", HO.NAMES)
def test_invariants(name):
    c, r = _select(name)
    ev = HO.evaluated(c["target"], c["K"])
    assert np.array_equal(r["n"], ev.reshape(c["B"], -1).sum(axis=1)) and (r["n"] > 0).all()
    assert np.array_equal(np.isnan(HO.case_cosine(name)), ~ev)
    assert np.array_equal(r["keep"], -(-r["n"] * HO.KEEP // 1000)) and (r["keep"] >= 1).all()
    for b in range(c["B"]):
        t = r["tmin"][b]
        assert 1 <= t <= HO.BINS
        assert r["prefix"][b, t] >= r["keep"][b] > r["prefix"][b, t - 1]          # the smallest t that reaches the budget
        assert r["cut"][b] == max(t, 512) and r["counts"][b, 0] == r["n"][b]
        assert r["counts"][b, 1] == r["prefix"][b, r["cut"][b]] >= r["keep"][b]
        kept = ev[b] & ~r["dropped"][b]
        assert kept.sum() == r["counts"][b, 1]
        # whole bins: every kept pixel lies below every dropped one
        q = HO.bins(HO.case_cosine(name)[b])
        assert q[kept].max() < r["cut"][b] <= q[r["dropped"][b]].min()
    out = r["target_out"]
    assert np.array_equal(out[~r["dropped"]], c["target"][~r["dropped"]]) and (out[r["dropped"]] == HO.DROP).all()
    assert r["dropped"].any() and not r["dropped"][~ev].any()


@pytest.mark.parametrize("name", HO.NAMES)
def test_both_branches_are_reached(name):
    """the precondition of the GPU tests: with keep 250 and thresh 0.0 the threshold bin 512 decides where tmin lies below it"""
    c, r = _select(name)
    if name in THRESHOLD_DRIVEN:
        assert (301 <= r["tmin"]).all() and (r["tmin"] <= 452).all() and (r["cut"] == 512).all()
        assert (r["counts"][:, 1] > r["keep"]).all()
    else:
        assert (608 <= r["tmin"]).all() and (r["tmin"] <= 776).all() and np.array_equal(r["cut"], r["tmin"])
    # the threshold off: the budget alone
    off = _select(name, thresh=HO.OFF)[1]
    assert np.array_equal(off["cut"], off["tmin"]) and np.array_equal(off["tmin"], r["tmin"])


@pytest.mark.parametrize("name", ["c1_s32_e5_k21", "c5_s8_e300_k59"])
def test_keep_everything_skip_and_empty_images(name):
    c, full = _select(name, keep=1000, thresh=HO.OFF)
    assert np.array_equal(full["target_out"], c["target"]) and not full["dropped"].any()
    assert np.array_equal(full["counts"][:, 0], full["counts"][:, 1])
    # keep = 1 permille still keeps one whole bin of every image
    one = _select(name, keep=1, thresh=HO.OFF)[1]
    assert (one["keep"] == 2).all() and (one["counts"][:, 1] >= 2).all()
    # a skip set: its pixels are neither counted nor dropped
    skip = c["unseen"]
    s = _select(name, skip=skip)[1]
    in_skip = np.isin(c["target"], skip)
    assert in_skip.any() and not s["dropped"][in_skip].any()
    assert np.array_equal(s["n"], (HO.evaluated(c["target"], c["K"]) & ~in_skip).reshape(c["B"], -1).sum(axis=1))
    # an image without a valid pixel: cut 0, counts {0, 0}, the target verbatim
    t = c["target"].copy()
    t[0] = -1
    e = HO.select(HO.case_cosine(name), t, c["K"], HO.KEEP, HO.THRESH)
    assert e["cut"][0] == 0 and not e["counts"][0].any() and np.array_equal(e["target_out"][0], t[0])
    assert e["cut"][1] > 0


def test_bins_and_threshold_edges():
    nan = np.float32("nan")
    assert list(HO.bins(np.array([nan, -1.0, -1.5, -1 / 512, 0.0, 1 / 512, 1.0 - 1e-7, 1.0, 1.5], dtype=np.float32))) == \
        [0, 0, 0, 511, 512, 513, 1023, 1023, 1023]
    assert [HO.thresh_bin(t) for t in (-2.0, -1.0, -1.0 + 1 / 512, 0.0, 0.001, 1 / 512, 1.0, 2.0, 1e38)] == \
        [0, 0, 1, 512, 512, 513, 1024, 1024, 1024]
    # a NaN pixel lands in bin 0, which every cut >= 1 keeps
    conf = np.array([[[nan, 0.9, 0.8, 0.1]]], dtype=np.float32)
    tgt = np.array([[[1, 1, 2, 0]]])
    r = HO.select(conf, tgt, 3, 250, HO.OFF)
    assert r["qhist"][0, 0] == 1 and r["tmin"][0] == 1 and r["cut"][0] == 1 and list(r["counts"][0]) == [4, 1]
    assert list(r["target_out"][0, 0]) == [1, HO.DROP, HO.DROP, HO.DROP]
    # thresh 1.0 -> bin 1024: everything is kept whatever the budget
    r = HO.select(conf, tgt, 3, 250, 1.0)
    assert r["cut"][0] == 1024 and list(r["counts"][0]) == [4, 4] and np.array_equal(r["target_out"], tgt)
