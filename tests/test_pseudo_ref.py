"""CPU: the numpy restatement of the pseudo-label contract (tests/helpers_pseudo.py) on the synthetic cases of helpers_calib -- the
properties the GPU test then relies on: few unclear pixels, the selection takes at least the asked share and at most one threshold bin
more, keep = 1 takes everything, nothing hidden -> nothing changes, classes without candidates get the threshold 1024, and the cases
cover both empty classes and several distinct thresholds."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers_calib as HC  # noqa: E402
import helpers_pseudo as HP  # noqa: E402


def _staged(name, gamma, keep=HP.KEEP):
    c = HC.case(name)
    cand, vb, unclear = HP.case_candidates(name, gamma)
    return c, cand, vb, unclear, HP.select(cand, vb.astype(np.float32), HP.target(name), c["K"], keep)


@pytest.mark.parametrize("gamma", HP.GAMMAS)
@pytest.mark.parametrize("name", HP.NAMES)
def test_reference_properties(name, gamma):
    c, cand, vb, unclear, r = _staged(name, gamma)
    tgt, K = HP.target(name), c["K"]
    hidden = tgt == HP.HIDDEN
    assert hidden.any() and (tgt == -1).any() and (tgt == -2).any() and not np.isin(tgt, c["unseen"]).any()
    share = unclear[hidden].mean()
    print("%s gamma %g: %d hidden pixels, %.2f %% unclear, %d candidates in %d of %d unseen classes, %d distinct thresholds"
          % (name, gamma, hidden.sum(), 100 * share, (cand >= 0).sum(), (r["counts"][:, 0] > 0).sum(), len(c["unseen"]),
             len(set(r["thr"][r["counts"][:, 0] > 0]))))
    assert share <= 0.05
    # candidates: hidden pixels only, unseen classes only, at or above the floor
    assert not (cand[~hidden] >= 0).any() and np.isin(cand[cand >= 0], c["unseen"]).all() and (vb[cand >= 0] >= HP.CONF_FLOOR).all()
    n, sel = r["counts"][:, 0], r["counts"][:, 1]
    assert np.array_equal(n, np.bincount(cand[cand >= 0], minlength=K)) and n.sum() > 0
    for k in range(K):
        if n[k] == 0:
            assert r["thr"][k] == HP.BINS and sel[k] == 0
            continue
        t = r["thr"][k]
        assert 0 <= t < HP.BINS and r["qhist"][k, t] > 0
        assert sel[k] >= r["keep"][k] and sel[k] - r["keep"][k] < r["qhist"][k, t]
        assert sel[k] == ((cand == k) & r["selected"]).sum()
    # the relabelled target: the selected pixels carry their class, everything else is the target
    out = r["target_out"]
    assert np.array_equal(out[~r["selected"]], tgt[~r["selected"]]) and np.array_equal(out[r["selected"]], cand[r["selected"]])
    assert r["selected"].sum() == sel.sum() and (out[~hidden] == tgt[~hidden]).all()


@pytest.mark.parametrize("name", HP.NAMES)
def test_keep_everything_and_nothing_hidden(name):
    c, cand, vb, _, r = _staged(name, 0.0, keep=1000)
    assert np.array_equal(r["selected"], cand >= 0) and np.array_equal(r["counts"][:, 0], r["counts"][:, 1])
    plain = np.where(HP.target(name) == HP.HIDDEN, -1, HP.target(name))          # no hidden pixel at all
    ref = HC.case_reference(name)
    cand0, vb0, _ = HP.candidates(ref, plain, 0.0, HP.CONF_FLOOR, ref["unclear"][8])
    assert (cand0 == -1).all()
    r0 = HP.select(cand0, vb0.astype(np.float32), plain, c["K"], HP.KEEP)
    assert np.array_equal(r0["target_out"], plain) and (r0["thr"] == HP.BINS).all() and not r0["counts"].any()


def test_the_cases_cover_empty_classes_and_distinct_thresholds():
    empty = several = 0
    for name in HP.NAMES:
        for gamma in HP.GAMMAS:
            c, _, _, _, r = _staged(name, gamma)
            has = r["counts"][c["unseen"], 0] > 0
            empty += int((~has).any())
            several += int(len(set(r["thr"][np.asarray(c["unseen"])[has]])) >= 3)
    assert empty > 0 and several > 0


def test_bins_are_the_float32_expression():
    conf = np.array([-1.0, -0.99999994, -0.001953125, 0.0, 0.001953125, 0.2, 0.99999994, 1.0, 1.5, -1.5], dtype=np.float32)
    assert HP.bins(conf).tolist() == [0, 0, 511, 512, 513, 614, 1023, 1023, 1023, 0]
    # c * 512 is a power-of-two scaling: exact, so fma(c, 512, 512) and the two-step float32 form agree
    rng = np.random.RandomState(5)
    c = rng.uniform(-1, 1, 100000).astype(np.float32)
    exact = np.floor(c.astype(np.float64) * 512 + 512)
    two_step = np.floor(c * np.float32(512) + np.float32(512))
    fused = np.floor((c.astype(np.float64) * 512 + 512).astype(np.float32))
    assert np.array_equal(two_step, fused) and (np.abs(two_step - exact) <= 1).all()
