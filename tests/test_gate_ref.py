"""CPU: the numpy restatement of the soft seen/unseen gate (tests/helpers_gate.py) is consistent with itself -- the crossing tables give
the direct histograms, D stays inside [-log n_U, log n_S], weight = 0 is the hard threshold on the true groups -- and the torch referee
utils.soft_gate_infer follows the same rule on a small materialised score."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers_gate as HG  # noqa: E402
import helpers_seen_sweep as HS  # noqa: E402


@pytest.mark.parametrize("kind", HS.UNSEEN_KINDS)
@pytest.mark.parametrize("name", HG.NAMES)
def test_crossing_tables_bounds_and_weight_zero(name, kind):
    c = HG.case(name)
    K, tgt = c["K"], c["target"]
    for temperature, weight in ((0.1, 1.0), (0.01, 4.0)):
        r = HG.reference(name, kind, temperature, weight)
        direct = HG.histograms(name, r)
        assert np.array_equal(HS.crossing_histograms(tgt, r["A"], r["Bc"], r["e64"], r["taus"], K), direct)
        live = ~r["dead"]
        assert r["dead"].any() and np.isfinite(r["D"][live]).all()
        assert (r["D"][live] >= -np.log(r["n_unseen"]) - 1e-12).all() and (r["D"][live] <= np.log(r["n_seen"]) + 1e-12).all()
        assert (r["pred"][:, r["dead"]] == 0).all()
        assert (r["pred"][0][live] == r["A"][live]).all() and (r["pred"][-1][live] == r["Bc"][live]).all()      # below / above every e
    # the gate is no cosmetic variant: at T = 0.1 it moves the group decision of a good share of the pixels against the hard cut at 0
    r = HG.reference(name, kind, 0.1, 1.0)
    with np.errstate(invalid="ignore"):
        moved = ((r["e64"] > 0) != (HG.sims(name)[2] > 0))[~r["dead"]].mean()
    print("%s %s: the soft rule changes the group of %.1f%% of the pixels at tau = 0" % (name, kind, 100 * moved))
    assert 0.2 < moved < 0.5
    # weight = 0: e is the margin, the rule is the hard threshold with the true in-group answers
    z = HG.reference(name, kind, 0.1, 0.0)
    m32 = HG.sims(name)[2]
    live = ~z["dead"]
    assert np.array_equal(z["e64"][live], m32.astype(np.float64)[live])
    want = HS.predict(z["A"], z["Bc"], m32, z["taus"])
    assert np.array_equal(z["pred"][:, live], want[:, live])


@pytest.mark.parametrize("kind", ["zero", "high"])
def test_one_class_per_group_has_no_correction(kind):
    for temperature, weight in ((0.1, 1.0), (0.01, 4.0)):
        r = HG.reference(HG.K2, kind, temperature, weight)
        live = ~r["dead"]
        assert (r["D"][live] == 0).all() and np.array_equal(r["e64"][live], HG.sims(HG.K2)[2].astype(np.float64)[live])
        assert (r["A"][live] == 1 - HG.unseen_of(HG.K2, kind)[0]).all() and (r["Bc"][live] == HG.unseen_of(HG.K2, kind)[0]).all()


def test_soft_gate_infer_follows_the_numpy_rule():
    from zeroshotsemanticsegmentation_amd import _lib as L, utils
    rng = np.random.RandomState(11)
    B, E, K, H, W = 2, 20, 21, 9, 11
    emb = HS.embeddings(E, K)
    score = rng.randn(B, E, H, W).astype(np.float32)
    score[0, :, 0, 0] = 0.0                                                   # a zero-norm pixel
    sm = rng.randn(B, 2, H, W).astype(np.float32)
    sm[1, 1, 2, 3] = np.nan                                                   # a NaN margin
    unseen = HS.unseen_sets(K)["half"]
    seen = [k for k in range(K) if k not in unseen]
    s64 = score.astype(np.float64).transpose(0, 2, 3, 1)
    with np.errstate(invalid="ignore"):
        sim = s64 @ emb.astype(np.float64).T / (np.linalg.norm(s64, axis=-1, keepdims=True) * np.linalg.norm(emb.astype(np.float64), axis=1))
    A, va, la = HG.HC.group_best(sim, seen)
    Bc, vb, lb = HG.HC.group_best(sim, unseen)
    for temperature, weight, tau in ((0.1, 1.0, 0.0), (0.01, 4.0, 0.5), (0.1, 0.0, -0.25)):
        D = HG.log_sum_exp(sim, seen, va, temperature) - HG.log_sum_exp(sim, unseen, vb, temperature)
        e = (sm[:, 1] - sm[:, 0]).astype(np.float64) - weight * D
        with np.errstate(invalid="ignore"):
            want = np.where(np.isnan(D), 0, np.where(e > tau, A, Bc))
            clear = ~((np.abs(e - tau) <= HG.bound(weight, temperature, e)) | (la <= HG.NEAR_TIE) | (lb <= HG.NEAR_TIE))
        got = utils.soft_gate_infer(torch.from_numpy(score), torch.from_numpy(sm), emb, unseen, tau, temperature, weight)
        assert got.dtype == torch.int64 and tuple(got.shape) == (B, H, W)
        got = got.numpy()
        assert clear.mean() > 0.9 and np.array_equal(got[clear], want[clear])
        assert got[0, 0, 0] == 0 and got[1, 2, 3] == Bc[1, 2, 3]
        assert 0 < (np.isin(got, unseen)).mean() < 1
    for bad in (dict(unseen=[]), dict(unseen=list(range(K))), dict(temperature=0.0), dict(temperature=float("nan")), dict(weight=-1.0),
                dict(weight=float("inf")), dict(embeddings=emb[:, :5])):
        kw = dict(score=torch.from_numpy(score), seen_mask_score=torch.from_numpy(sm), embeddings=emb, unseen=unseen, tau=0.0,
                  temperature=0.1, weight=1.0)
        kw.update(bad)
        with pytest.raises(L.SznError):
            utils.soft_gate_infer(**kw)
