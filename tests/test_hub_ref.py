"""CPU: the torch-op referee of the hubness correction (utils.hub_infer) against the numpy float64 restatement in tests/helpers_hub.py,
its beta = 0 identity, utils.hubness_skew on hand-made histograms, the effect on a constructed hub, and the share of pixels the GPU test
will leave out as unclear (float64 reference alone)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers_calib as HC  # noqa: E402
import helpers_hub as HH  # noqa: E402
import helpers_msinfer as HM  # noqa: E402
from zeroshotsemanticsegmentation_amd import _lib as L, utils  # noqa: E402


def _score(c):
    """the (B,E,H,W) fp32 score a model would materialise for case c"""
    s = HM.up_crop(c["coarse"], c["S"], c["H"], c["W"], HM.CROP[c["S"]])
    return torch.from_numpy(np.ascontiguousarray(s.transpose(0, 3, 1, 2)).astype(np.float32))


@pytest.mark.parametrize("mode", HH.MODES)
@pytest.mark.parametrize("name", ["c1_s32_e5_k21", "c3_s8_e20_k33", "c4_s32_e20_k70"])
def test_hub_infer_against_float64_on_the_clear_pixels(name, mode):
    c = HC.case(name)
    ref = HH.case_reference(name, mode)
    gam = HH.gammas(mode)
    score, emb = _score(c), torch.from_numpy(c["emb"])
    valid = torch.from_numpy(c["target"] != HH.PAD)
    compared = 0
    for gi in (0, 5, 8, 12, 16):
        got = utils.hub_infer(score, emb, c["unseen"], mode, HH.BETA, float(gam[gi]), HH.MIN_SD, valid).numpy()
        clear = ~ref["unclear"][gi]
        assert got.shape == (c["B"], c["H"], c["W"]) and got.dtype == np.int64
        assert np.array_equal(got[clear], ref["pred"][gi][clear]), gi
        compared += int(clear.sum())
    assert compared > 0.8 * 5 * got.size
    # the statistics see `valid`: without it the padding rows move the means, and some prediction with them
    ok_all = HH.counted(HC.case_reference(name)["sim"])
    assert ok_all.sum() > HH.case_moments(name)[0].sum()


def _plain(score, emb, unseen, gamma):
    """calibrated stacking's rule on the uncorrected cosines, hub_infer's own operations"""
    K = emb.shape[0]
    is_unseen = torch.zeros(K, dtype=torch.bool)
    is_unseen[list(unseen)] = True
    seen_idx, unseen_idx = torch.nonzero(~is_unseen)[:, 0], torch.nonzero(is_unseen)[:, 0]
    sim = torch.einsum('behw,ke->bkhw', score, emb) / (score.norm(dim=1, keepdim=True) * emb.norm(dim=1).view(1, K, 1, 1))
    a, va = utils._first_max(sim, seen_idx)
    b, vb = utils._first_max(sim, unseen_idx)
    m = va - vb
    g = float(np.float32(gamma))
    pred = torch.where((m > g) | ((m == g) & (a < b)), a, b)
    return torch.where(torch.isnan(m), torch.zeros_like(pred), pred)


def test_beta_zero_in_mean_mode_is_the_plain_calibrated_rule_exactly():
    c = HC.case("c3_s8_e20_k33")
    score, emb = _score(c), torch.from_numpy(c["emb"])
    score[0, :, 4:9, 10:20] = 0.0                                 # zero-norm pixels: class 0 in both
    for g in (-0.25, 0.0, 0.125):
        plain = _plain(score, emb, c["unseen"], g)
        got = utils.hub_infer(score, emb, c["unseen"], "mean", 0.0, g)
        assert torch.equal(got, plain)
        assert (got[0, 4:9, 10:20] == 0).all()
    assert not torch.equal(utils.hub_infer(score, emb, c["unseen"], "mean", 1.0, 0.0), _plain(score, emb, c["unseen"], 0.0))
    for bad in (dict(mode="median"), dict(beta=-1.0), dict(beta=float("nan")), dict(min_sd=0.0), dict(unseen=[]), dict(unseen=[33])):
        kw = dict(dict(unseen=c["unseen"], mode="mean", beta=1.0, min_sd=0.05), **bad)
        with pytest.raises(L.SznError):
            utils.hub_infer(score, emb, kw["unseen"], kw["mode"], kw["beta"], 0.0, kw["min_sd"])


def test_hubness_skew_on_hand_made_histograms():
    assert utils.hubness_skew(np.full((4, 4), 3)) == 0.0                      # every class predicted equally often
    assert utils.hubness_skew(np.zeros((5, 5))) == 0.0
    # the column sums count: N_k = (10, 1, 1, 1) whatever the rows
    h = np.array([[4, 1, 0, 0], [3, 0, 1, 0], [2, 0, 0, 1], [1, 0, 0, 0]])
    nk = np.array([10.0, 1.0, 1.0, 1.0])
    d = nk - nk.mean()
    want = (d ** 3).mean() / (d * d).mean() ** 1.5
    assert abs(utils.hubness_skew(h) - want) < 1e-12 and abs(want - 2 / np.sqrt(3)) < 1e-12
    assert abs(utils.hubness_skew(nk) - want) < 1e-12                         # a vector of counts is taken as N_k
    assert abs(utils.hubness_skew(h.T[::-1]) - HH.skew(h.T[::-1].sum(axis=0))) < 1e-12
    # one starved class among equals: negative; symmetric counts: zero
    assert utils.hubness_skew(np.diag([5, 5, 5, 0])) < 0
    assert abs(utils.hubness_skew(np.array([1, 2, 3, 4, 5]))) < 1e-12
    assert utils.hubness_skew(np.diag([9, 1, 1, 1, 1, 1])) > utils.hubness_skew(np.diag([3, 2, 1, 1, 1, 1])) > 0


def test_correction_reduces_the_skew_of_a_constructed_hub():
    """every pixel is its own class's vector plus a large share of class 3's: class 3 is close to every pixel and takes most of them;
    its mean similarity is what the correction takes off"""
    rng = np.random.RandomState(7)
    K, E, H, W, hubk = 12, 16, 24, 30, 3
    emb = rng.randn(K, E).astype(np.float32)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    cls = rng.randint(0, K, (1, H, W))
    s = emb[cls] + 1.3 * emb[hubk] + 0.2 * rng.randn(1, H, W, E).astype(np.float32)
    score = torch.from_numpy(np.ascontiguousarray(s.transpose(0, 3, 1, 2)).astype(np.float32))
    unseen = [2, 5, 8]
    plain = utils.hub_infer(score, torch.from_numpy(emb), unseen, "mean", 0.0).numpy()
    skews = {"plain": utils.hubness_skew(np.bincount(plain.ravel(), minlength=K))}
    for mode in HH.MODES:
        pred = utils.hub_infer(score, torch.from_numpy(emb), unseen, mode, 1.0).numpy()
        skews[mode] = utils.hubness_skew(np.bincount(pred.ravel(), minlength=K))
        assert (pred == cls).mean() > (plain == cls).mean() + 0.2
    print(skews)
    assert (plain == hubk).mean() > 0.5 and skews["plain"] > 2.0
    assert skews["mean"] < 0.5 * skews["plain"] and skews["zscore"] < 0.5 * skews["plain"]


@pytest.mark.parametrize("name,mode", HH.PRED_PAIRS)
def test_share_of_unclear_pixels_with_the_float64_table(name, mode):
    """what the GPU prediction test leaves out, with the float64 reference alone: at most 0.10 of the pixels unclear at some gamma"""
    ref = HH.case_reference(name, mode)
    share = ref["unclear"].any(axis=0).mean()
    print("%s %s: %.4f of the pixels unclear at some gamma" % (name, mode, share))
    assert 0 < share <= 0.10
    # the sweep moves pixels from the seen to the unseen group
    n_unseen = [np.isin(p, HC.case(name)["unseen"]).sum() for p in ref["pred"]]
    assert (np.diff(n_unseen) >= 0).all() and n_unseen[0] < n_unseen[-1]


def test_the_left_out_pair_is_the_crowded_one():
    ref = HH.case_reference("c2_s32_e300_k59", "zscore")
    share = ref["unclear"].any(axis=0).mean()
    print("c2_s32_e300_k59 zscore: %.4f unclear" % share)
    assert share > 0.10
