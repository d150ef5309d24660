"""CPU: the float64 restatement of the multi-scale inference contract (tests/helpers_msinfer.py) is itself checked -- against the
oracle's single-view head, against its own symmetries, and on a hand-made group case -- and the synthetic cases of the GPU tests meet
the conditions those tests put on their inputs (kappa <= 2, at most 5 % of the pixels inside the margin)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers_msinfer as HM  # noqa: E402
from oracle import szn_oracle as O  # noqa: E402


def _coarse(seed, B, h, w, E):
    return (np.random.RandomState(seed).rand(B, h, w, E) + 0.5).astype(np.float32)


def test_identity_view_reproduces_the_oracles_single_view_sims():
    B, h, w, E, H, W = 2, 2, 2, 20, 33, 47
    c = _coarse(1, B, h, w, E)
    emb = HM.embeddings(E, 33)
    sim, _ = HM.view_sims(c, 32, H, W, H, W, False, emb)
    # the oracle's upscore + crop (fp32), then szn_embed_argmax's formula in float64
    score = O.deconv_fwd(np.ascontiguousarray(c.transpose(0, 3, 1, 2)), 
                         np.broadcast_to(O.get_upsampling_weight(1, 1, 64)[0, 0], (E, 64, 64)), H, W, crop=19, diag=True)
    s = score.astype(np.float64).transpose(0, 2, 3, 1)
    want = (s @ emb.astype(np.float64).T) / (np.linalg.norm(s, axis=3)[..., None] * np.linalg.norm(emb.astype(np.float64), axis=1))
    assert np.abs(sim - want).max() < 1e-6
    # and the prediction is the oracle's nearest class wherever the float64 margin is not at fp32 rounding level
    ref = HM.reference(32, H, W, [(c, H, W, False)], emb)
    clear = ref["margin"] > 1e-5
    assert clear.mean() > 0.95
    assert np.array_equal(ref["pred"][clear], O.infer_lbl(score, emb)[clear])
    # stride 8: the fused-head oracle's prediction
    c8 = _coarse(2, B, 14, 14, E)
    ref8 = HM.reference(8, H, W, [(c8, H, W, False)], emb)
    _, _, p8, _ = O.fused_head(c8, emb, None, H, W, crop=31, want_grad=False, stride=8)
    clear = ref8["margin"] > 1e-5
    assert clear.mean() > 0.95 and np.array_equal(ref8["pred"][clear], p8[clear])


def test_copies_of_one_view_sum():
    c = _coarse(3, 1, 2, 3, 5)
    emb = HM.embeddings(5, 21)
    one = HM.reference(32, 33, 47, [(c, 50, 71, True)], emb)
    three = HM.reference(32, 33, 47, [(c, 50, 71, True)] * 3, emb)
    assert np.allclose(three["acc"], 3 * one["acc"], rtol=1e-14, atol=0)
    assert np.array_equal(three["kappa"], one["kappa"])


def test_constant_map_gives_view_independent_sims():
    emb = HM.embeddings(5, 21)
    vec = np.array([0.7, 1.1, 0.9, 1.3, 0.6], dtype=np.float32)
    sims = []
    for Hs, Ws, flip in HM.view_sizes(33, 47, HM.SCALES, True):
        # (interior pixels only see the constant: the map is made wide enough that no tap falls outside it)
        c = np.broadcast_to(vec, (1, HM.coarse_size(Hs, 32) + 2, HM.coarse_size(Ws, 32) + 2, 5)).copy()
        sim, kappa = HM.view_sims(c, 32, 33, 47, Hs, Ws, flip, emb, crop=32)
        assert np.allclose(kappa, 1.0, rtol=1e-12)
        sims.append(sim)
    for s in sims[1:]:
        assert np.allclose(s, sims[0], rtol=0, atol=1e-13)


def test_flip_of_a_flip_is_the_identity():
    for n_dst, n_src in ((47, 24), (47, 71), (47, 47), (24, 47)):
        i0, i1, w = HM.axis_map(n_dst, n_src)
        f0, f1, fw = HM.axis_map(n_dst, n_src, flip=True)
        assert np.array_equal(f0[::-1], i0) and np.array_equal(f1[::-1], i1) and np.array_equal(fw[::-1], w)
    x = np.random.RandomState(4).rand(2, 3, 9, 13).astype(np.float32)
    assert np.array_equal(HM.resize_flip(x, 9, 13), x)
    once = HM.resize_flip(x, 9, 13, flip=True)
    assert np.array_equal(once, x[..., ::-1])
    assert np.array_equal(HM.resize_flip(once, 9, 13, flip=True), x)
    # a mirrored view is the plain view read from the right: the same taps and weights, in reverse order
    assert np.array_equal(HM.resize_flip(x, 5, 20, flip=True), HM.resize_flip(x, 5, 20)[..., ::-1])


def test_group_rule_by_hand():
    # one image of 2 x 2 pixels, 4 classes, classes 1 and 3 unseen
    acc = np.array([[[[0.2, 0.9, 0.5, 0.1], [-0.3, 0.4, -0.1, 0.8]],
                     [[-0.5, 0.7, -0.2, 0.6], [np.nan, 0.3, 0.1, 0.2]]]])
    unseen = [1, 3]
    gmap = np.array([[[1, 0], [1, 0]]])                       # 0 = take the unseen group
    grp = HM.in_group(4, unseen, 1, gmap=gmap)
    pred = HM.group_pred(acc, grp)
    # (0,0) seen group: 0.2, 0, 0.5, 0 -> 2;  (0,1) unseen group: 0, 0.4, 0, 0.8 -> 3
    # (1,0) seen group, all of it negative: -0.5, 0, -0.2, 0 -> the out-of-group 0 of class 1 wins
    # (1,1) unseen group with a NaN at class 0 outside it: 0, 0.3, 0, 0.2 -> 1
    assert pred.tolist() == [[[2, 3], [1, 1]]]
    m = HM.margin(acc, grp)
    assert np.allclose(m, [[[0.3, 0.4], [0.2, 0.1]]])
    # mode 2: the group comes from the label; negative labels take the seen group
    target = np.array([[[1, 3], [-1, -2]]])
    grp2 = HM.in_group(4, unseen, 2, target=target)
    assert HM.group_pred(acc, grp2).tolist() == [[[1, 3], [1, 0]]]       # (1,1): the NaN of class 0 is in the seen group
    # mode 0: everything competes; a NaN in front keeps class 0
    assert HM.group_pred(acc, HM.in_group(4, unseen, 0, shape=acc.shape[:3])).tolist() == [[[1, 3], [1, 0]]]


@pytest.mark.parametrize("name", sorted(HM.CASES))
def test_gpu_cases_meet_their_input_conditions(name):
    c = HM.case(name)
    for mode in (0, 1, 2):
        ref = HM.case_reference(name, mode)
        assert np.nanmax(ref["kappa"]) <= 2.0
        excluded = ref["margin"] <= 2 * HM.bound(len(c["views"]), ref["kappa"], c["E"])
        print("%s mode %d: kappa max %.4f, bound max %.3e, %.2f %% of the pixels inside the margin"
              % (name, mode, np.nanmax(ref["kappa"]), HM.bound(len(c["views"]), ref["kappa"], c["E"]).max(), 100 * excluded.mean()))
        assert excluded.mean() <= 0.05
