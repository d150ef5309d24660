"""CPU: the float64 restatement of the ConSE contract (tests/helpers_conse.py) is sound on the shared cases -- few pixels are unclear,
so the GPU tests decide almost everywhere -- and the torch-op referee utils.conse_infer agrees with it on CPU tensors."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers_conse as HX  # noqa: E402


@pytest.mark.parametrize("name", HX.NAMES)
def test_few_pixels_are_unclear(name):
    ref = HX.case_reference(name)
    share = HX.unclear_share(ref)
    print("%s: unclear share %.4f%%, gap bound %.3g, median bound %.3g" % (name, 100 * share, np.median(ref["gap_bound"]), np.median(ref["bound"])))
    assert share <= HX.UNCLEAR_CAP
    assert ref["shaky"].mean() <= HX.UNCLEAR_CAP


def _score(c):
    """the materialised (B,K,H,W) float32 score of a case"""
    return torch.from_numpy(HX.HM.up_crop(c["coarse"], c["S"], c["H"], c["W"], HX.HM.CROP[c["S"]]).astype(np.float32)).permute(0, 3, 1, 2)


@pytest.mark.parametrize("name", HX.NAMES)
def test_referee_agrees_with_the_restatement(name):
    from zeroshotsemanticsegmentation_amd import utils
    c, ref = HX.case(name), HX.case_reference(name)
    score = _score(c)
    for g in (0, 8, 16):
        pred = utils.conse_infer(score, c["emb"], c["unseen"], c["T"], gamma=float(c["gammas"][g])).numpy()
        clear = ~ref["unclear"][g]
        assert pred.dtype == np.int64 and np.array_equal(pred[clear], ref["pred"][g][clear]), (name, g)
    got = utils.conse_infer(score, c["emb"], c["unseen"], c["T"], target=torch.from_numpy(c["target"])).numpy()
    want = HX.forced(ref["a"], ref["b"], ref["m"], c["target"], c["unseen"])
    clear = ~ref["shaky"]
    assert np.array_equal(got[clear], want[clear])


def test_top_1_at_gamma_0_predicts_the_top_seen_class():
    c = HX.case("c1_s32_e5_k21_t1")
    ref = HX.case_reference("c1_s32_e5_k21_t1")
    seen = np.array([k for k in range(c["K"]) if k not in c["unseen"]])
    top_seen = seen[HX.HM.first_argmax(ref["z"][..., seen])]
    assert np.array_equal(ref["top"][..., 0], top_seen)
    # f is that class's own embedding: cosine 1 with it, below 1 with every other row
    assert np.array_equal(ref["a"], top_seen)
    assert np.array_equal(ref["pred"][8], top_seen)


@pytest.mark.parametrize("name", HX.NAMES)
def test_unseen_share_grows_with_gamma(name):
    c, ref = HX.case(name), HX.case_reference(name)
    share = np.isin(ref["pred"], c["unseen"]).reshape(len(c["gammas"]), -1).mean(axis=1)
    assert (np.diff(share) >= 0).all() and share[-1] > share[0]


def test_forced_is_where_target_unseen_b_else_a():
    c, ref = HX.case("c4_s8_e20_k33_t5"), HX.case_reference("c4_s8_e20_k33_t5")
    out = HX.forced(ref["a"], ref["b"], ref["m"], c["target"], c["unseen"])
    hit = np.isin(c["target"], c["unseen"])
    assert hit.any() and (~hit).any()
    assert np.array_equal(out[hit], ref["b"][hit]) and np.array_equal(out[~hit], ref["a"][~hit])
    assert np.isin(out[hit], c["unseen"]).all() and not np.isin(out[~hit], c["unseen"]).any()
    # the same through the gamma rule: a large gamma always takes b, a large negative one a
    far = HX.HC.predict(ref["a"], ref["b"], ref["m"], np.array([-4.0, 4.0], dtype=np.float32))
    assert np.array_equal(out, np.where(hit, far[1], far[0]))


def test_referee_refuses_bad_arguments():
    from zeroshotsemanticsegmentation_amd import _lib as L, utils
    score, emb = torch.zeros(1, 6, 2, 2), torch.ones(6, 3)
    for kw in (dict(unseen=[], top_t=2), dict(unseen=range(6), top_t=2), dict(unseen=[6], top_t=2), dict(unseen=[1], top_t=0)):
        with pytest.raises(L.SznError):
            utils.conse_infer(score, emb, **kw)
    with pytest.raises(L.SznError):
        utils.conse_infer(score, torch.ones(5, 3), [1], 2)
