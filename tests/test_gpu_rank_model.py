"""GPU: the hinge ranking loss through the layers that key off "an embedding loss with a fused head" -- hard-pixel mining and pseudo
labels on engine.TrainStep(loss="rank"), and the models' calibrated, multi-scale and seen-mask-threshold predict methods -- on
B = 2, 64 x 64, E = 20, K = 21 with three unseen classes."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zeroshotsemanticsegmentation_amd import _lib as L  # noqa: E402
from zeroshotsemanticsegmentation_amd import datasets, engine, models, synth  # noqa: E402

E, K, B, H, W = 20, 21, 2, 64, 64
UNSEEN = [2, 5, 8]
HIDDEN = datasets.HIDDEN_LABEL
EMB = synth.make_embeddings(K, E)
RANK = dict(loss="rank", sim_exclude=UNSEEN, rank_margin=0.2)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def batch(hide=False):
    x = synth.make_images(B, H, W, seed=61)
    t = synth.make_labels(B, H, W, K, seed=62, block=8)
    t[:, -3:, :] = datasets.PAD_LABEL
    if hide:
        t[np.isin(t, UNSEEN)] = HIDDEN
    return cu(x), cu(t)


def fresh(**kw):
    m = models.FCN32s(E).load_synthetic(1337, device=torch.device("cuda")).eval()
    ts = engine.TrainStep(m, EMB, optimizer="adam", lr=1e-5, precision=torch.float32, **kw)
    ts.keep_ctx = True
    return ts


def _launches(monkeypatch, ts, x, t):
    names = []
    real = L.call

    def call(name, *a):
        names.append(name)
        return real(name, *a)
    with monkeypatch.context() as mp:
        mp.setattr(L, "call", call)
        lossv, pred = ts.step(x, t)
    torch.cuda.synchronize()
    return names, float(lossv), pred.clone()


def test_rank_step_with_ohem(monkeypatch):
    x, t = batch()
    excl = torch.isin(t, cu(np.array(UNSEEN)))
    assert excl.any()
    plain = _launches(monkeypatch, fresh(**RANK), x, t)
    assert "szn_fused_rank_head_prepared" in plain[0] and np.isfinite(plain[1])
    ts = fresh(ohem=dict(keep=0.25), **RANK)
    names, lossv, _ = _launches(monkeypatch, ts, x, t)
    assert np.isfinite(lossv) and "szn_ohem_head" in names and "szn_fused_rank_head_prepared" in names
    tp = ts.last_ohem_target
    assert torch.equal(tp[excl], t[excl]) and (tp != t).any()                  # labels in the exclude set: neither counted nor dropped
    assert int(ts.ohem_counts[0]) == int(((t >= 0) & ~excl).sum())
    assert torch.equal(ts.stats[:, 1], ((tp >= 0) & ~excl).sum(dim=(1, 2)).float())
    # inactive: the plain rank step, launch for launch and bit for bit
    off = fresh(ohem=dict(keep=0.25), **RANK)
    off.set_ohem_active(False)
    got = _launches(monkeypatch, off, x, t)
    assert got[0] == plain[0] and got[1] == plain[1] and torch.equal(got[2], plain[2])


def test_rank_step_with_pseudo_labels(monkeypatch):
    x, t = batch(hide=True)
    plain = _launches(monkeypatch, fresh(**RANK), x, t)
    ts = fresh(pseudo=dict(unseen=UNSEEN, gamma=2.5, keep=0.3, conf_floor=-2.0), **RANK)
    assert ts._sim_kw["exclude"] == []                                         # active: the unseen classes have positives now
    names, lossv, _ = _launches(monkeypatch, ts, x, t)
    assert np.isfinite(lossv) and "szn_pseudo_head" in names and "szn_fused_rank_head_prepared" in names
    tp = ts.last_pseudo_target
    n_seen = (t >= 0).sum(dim=(1, 2)).float()
    n_sel = (tp != t).sum(dim=(1, 2)).float()
    assert n_sel.sum() > 0 and torch.equal(ts.stats[:, 1], n_seen + n_sel)     # the pseudo-labelled pixels count
    ts.set_pseudo_active(False)
    assert ts._sim_kw["exclude"] == UNSEEN
    off = fresh(pseudo=dict(unseen=UNSEEN, gamma=2.5, keep=0.3), **RANK)
    off.set_pseudo_active(False)
    got = _launches(monkeypatch, off, x, t)
    assert got[0] == plain[0] and got[1] == plain[1] and torch.equal(got[2], plain[2])


@pytest.mark.parametrize("arch", ["fcn32s", "fcn8s"])
def test_predict_methods_take_rank_and_keep_the_cosine_prediction(arch):
    x, t = batch()
    cls = models.FCN32s if arch == "fcn32s" else models.FCN8s
    m = cls(E).load_synthetic(1337, device=torch.device("cuda")).eval().set_rank(UNSEEN, 0.2, True)
    with torch.no_grad():
        want_loss = m.embed_predict(x, EMB, t, loss="rank")[0].clone()
    assert torch.isfinite(want_loss) and float(want_loss) > 0
    gammas = np.linspace(0.0, 0.4, 5).astype(np.float32)
    taus = np.linspace(-1.0, 1.0, 5).astype(np.float32)
    calls = {
        "calib": lambda loss: m.calib_predict(x, EMB, UNSEEN, gammas, t, pred_index=2, loss=loss),
        "ms": lambda loss: m.ms_predict(x, EMB, [0.5, 1.0], True, t, loss=loss),
        "seen_sweep": lambda loss: m.seen_sweep_predict(x, EMB, UNSEEN, taus, t, pred_index=2, loss=loss),
    }
    for name, fn in calls.items():
        r = [v.clone() if isinstance(v, torch.Tensor) else v for v in fn("rank")]
        c = fn("cos")
        assert torch.equal(r[1], c[1]), name                                   # the prediction: the cosine head's, bit for bit
        if len(r) > 2 and r[2] is not None:
            assert torch.equal(r[2], c[2]), name                               # and so the histograms
        assert torch.equal(r[0], want_loss), name                              # the loss: embed_predict(loss="rank")'s on that map
        assert not torch.equal(r[0], c[0]), name
    lr, pr = m.szn_predict_rank(x, EMB, UNSEEN, t)
    lr, pr = lr.clone(), pr.clone()
    lc, pc = m.szn_predict(x, EMB, UNSEEN, t)
    assert torch.equal(pr, pc) and torch.equal(lr, want_loss)
