"""CPU: the numpy restatement of the seen-mask threshold sweep (tests/helpers_seen_sweep.py) against the oracle's seen-mask-stitched
inference at tau = 0, its own invariants over ascending taus, and the share of pixels the synthetic cases leave to the near-tie rule."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers_msinfer as HM  # noqa: E402
import helpers_seen_sweep as HS  # noqa: E402
from oracle import szn_oracle as O  # noqa: E402

U = 2.0 ** -24


@pytest.mark.parametrize("name", HS.NAMES)
def test_tau_zero_is_the_oracles_stitched_inference(name):
    c, ref = HS.case(name), HS.case_reference(name)
    # the oracle's route: the materialised embedding score and the materialised (B,2,H,W) seen-mask score, stitched per pixel
    score = HM.up_crop(c["fmap"], c["S"], c["H"], c["W"], HM.CROP[c["S"]]).transpose(0, 3, 1, 2).astype(np.float32)
    sm_score = O.deconv_fwd(c["sm"].transpose(0, 3, 1, 2), c["wt"], c["H"], c["W"], crop=HS.CROP)
    m64, mag = HS.margin64(c["sm"], c["wt"], c["H"], c["W"])
    decided = np.abs(m64) > 16 * U * mag                 # elsewhere two fp32 orders of the 16 products may disagree about the sign
    assert np.array_equal((ref["m32"] > 0)[decided], (sm_score[:, 1] > sm_score[:, 0])[decided])
    assert np.array_equal((ref["m32"] > 0)[decided], (m64 > 0)[decided])
    for kind, unseen in HS.unseen_sets(c["K"]).items():
        A, Bc, unclear = ref[kind]
        want = O.infer_lbl_szn(score, sm_score, c["emb"], unseen)
        got = HS.predict(A, Bc, ref["m32"], [0.0])[0]
        ok = decided & ~unclear & ~ref["dead"]            # (a zero-norm pixel of the materialised fp32 score need not be one)
        assert ok.mean() > 0.85 and (~(decided & ~unclear)).mean() < 0.01, (kind, ok.mean())
        assert np.array_equal(got[ok], want[ok]), (kind, int((got[ok] != want[ok]).sum()))


@pytest.mark.parametrize("name", HS.NAMES)
def test_margin32_is_within_the_bound_of_margin64(name):
    c, ref = HS.case(name), HS.case_reference(name)
    m64, mag = HS.margin64(c["sm"], c["wt"], c["H"], c["W"])
    # 8 fmas per channel and one subtraction: each rounds a partial sum bounded by the sum of the |products|
    assert (np.abs(ref["m32"].astype(np.float64) - m64) <= 16 * U * mag).all()
    assert (HS.margin32(np.zeros_like(c["sm"]), c["wt"], c["H"], c["W"]) == 0).all()
    sym = c["wt"].copy()
    sym[:, 1] = sym[:, 0]
    both = np.repeat(c["sm"][..., :1], 2, axis=3)
    assert (HS.margin32(both, sym, c["H"], c["W"]) == 0).all()


@pytest.mark.parametrize("n_taus", [1, 64])
@pytest.mark.parametrize("name", HS.NAMES)
def test_histograms_over_ascending_taus(name, n_taus):
    c, ref = HS.case(name), HS.case_reference(name)
    K, t, m = c["K"], c["target"], ref["m32"]
    taus = HS.taus_from(m, n_taus)
    assert taus.size == n_taus and (np.diff(taus) > 0).all()
    assert (m[..., None] == taus).any()                                        # equality margin == tau occurs (it means "unseen")
    counted = (t >= 0) & (t < K)
    assert (t == -1).any() and (t == -2).any() and (t >= K).any()
    for kind in HS.UNSEEN_KINDS:
        A, Bc, _ = ref[kind]
        pred = HS.predict(A, Bc, m, taus)
        hist = HS.histograms(t, pred, K)
        assert np.array_equal(hist, HS.crossing_histograms(t, A, Bc, m, taus, K))
        # every histogram counts the same pixels per target class
        assert (hist.sum(axis=2) == np.bincount(t[counted], minlength=K)[None]).all()
        b = HS.bins(m, taus)
        if n_taus == 64:
            assert (b == 0).sum() == 0 and (b == n_taus).sum() == 0            # the first tau lies below, the last above every margin
            assert np.array_equal(pred[0], A) and np.array_equal(pred[-1], Bc)
        for g in range(n_taus - 1):
            moved = pred[g] != pred[g + 1]
            # raising tau moves pixels only from A to Bc, and exactly those whose bin is g + 1
            assert np.array_equal(pred[g][moved], A[moved]) and np.array_equal(pred[g + 1][moved], Bc[moved])
            assert np.array_equal(moved, (b == g + 1) & (A != Bc))
            step = np.zeros((K, K), dtype=np.int64)
            sel = moved & counted
            np.add.at(step, (t[sel], Bc[sel]), 1)
            np.add.at(step, (t[sel], A[sel]), -1)
            assert np.array_equal(hist[g + 1] - hist[g], step)
        n_seen_group = (m[None] > taus.reshape(-1, 1, 1, 1)).sum(axis=(1, 2, 3))
        assert (np.diff(n_seen_group) <= 0).all()


@pytest.mark.parametrize("name", HS.NAMES)
def test_the_cases_hold_what_the_gpu_tests_need(name):
    c, ref = HS.case(name), HS.case_reference(name)
    sets = HS.unseen_sets(c["K"])
    assert ref["dead"].any() and ref["dead"].mean() < 0.15                     # zero-norm pixels
    for kind in HS.UNSEEN_KINDS:
        A, Bc, unclear = ref[kind]
        print("%s %s: %.3f %% of the pixels within %g of a tie" % (name, kind, 100 * unclear.mean(), HS.NEAR_TIE))
        assert unclear.mean() < 0.01
        assert (A[ref["dead"]] == 0).all() and (Bc[ref["dead"]] == 0).all()
    # {0} unseen: in the unseen group class 0 wins with a positive cosine, else the first zeroed row, class 1
    assert set(np.unique(ref["zero"][1])) == {0, 1}
    # all but two classes unseen: a pixel with a negative cosine to both seen classes answers with the first zeroed row in the seen group
    A = ref["most"][0]
    assert set(np.unique(A)) == {0, 3, 7} and (np.isin(A, sets["most"]) & ~ref["dead"]).mean() > 0.05
    assert (ref["high"][1] != c["K"] - 1).any() and (ref["high"][1] == c["K"] - 1).any()
