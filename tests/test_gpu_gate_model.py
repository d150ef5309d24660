"""GPU: the soft seen/unseen gate through the model surface (FCN32s / FCN8s .seen_gate_predict) and the trainer (seen_gate=,
validate(True)), on a tiny synthetic set (64 x 64 images, 33 classes, E = 20)."""
import functools
import os
import pathlib
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zeroshotsemanticsegmentation_amd import _lib as L  # noqa: E402
from zeroshotsemanticsegmentation_amd import heads, models, optim, synth, trainer_fcn, utils  # noqa: E402
from zeroshotsemanticsegmentation_amd.synthetic_dataset import SyntheticSegmentation  # noqa: E402

E, K, B, H, W = 20, 33, 2, 64, 64
UNSEEN = [0, 12, 15, 24]
VAL_UNSEEN = [15, 24]
EMB = np.load(os.path.join(ROOT, "tests", "golden", "embeddings_context_20.npy"))
KINDS = {"fcn32s": models.FCN32s, "fcn8s": models.FCN8s}
GATE = dict(weight=1.0, temperature=0.1)


@functools.lru_cache(maxsize=None)
def net(kind):
    return KINDS[kind](E).load_synthetic(1337, device=torch.device("cuda")).eval()


@functools.lru_cache(maxsize=None)
def batch():
    x = torch.from_numpy(synth.make_images(B, H, W, seed=31)).cuda()
    t = synth.make_labels(B, H, W, K, seed=32, block=8)
    t[:, :2, :3] = -1
    return x, torch.from_numpy(t).cuda()


def _pixel(kind, gate=True):
    return ("gate" if gate else "sweep") + ("_cell_kernel" if kind == "fcn32s" else "_cell_tab_kernel")


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_seen_gate_predict(kind):
    m = net(kind)
    x, t = batch()
    taus = np.linspace(-1.0, 1.0, 5).astype(np.float32)
    loss0, pred0, hist0 = m.seen_sweep_predict(x, EMB, UNSEEN, taus, t, pred_index=2)
    assert hist0 is None and L.last_kernel() == _pixel(kind, False)
    # the gate: the loss of the plain route bit for bit, on the same workspace reuse path (a prediction-only call: no histogram kernel)
    loss, pred, hist = m.seen_gate_predict(x, EMB, UNSEEN, taus, GATE, t, pred_index=2)
    assert hist is None and L.last_kernel() == _pixel(kind) and L.prev_kernel() == "smh_margin_kernel" and m._last_pred is pred
    assert torch.equal(loss, loss0) and loss.dim() == 0
    margin = m._last_margin.clone()
    assert margin.dtype == torch.float32 and tuple(margin.shape) == (B, H, W)
    # pred and hist are a direct heads.soft_gate call's on the kept map and margin
    _, stride, fmap = m._head_map(x)
    fmap = fmap.float().clone()                      # (the next forward pass reuses the engine's buffers)
    emb = torch.from_numpy(EMB).cuda()
    want_hist, want_pred, eff = heads.soft_gate(stride, fmap, emb, H, W, UNSEEN, margin, taus, GATE["temperature"], GATE["weight"], t,
                                                pred_index=2, want_eff=True)
    assert torch.equal(pred, want_pred)
    hist = torch.zeros(len(taus), K, K, dtype=torch.int64, device="cuda")
    loss2, pred2, hist2 = m.seen_gate_predict(x, EMB, UNSEEN, taus, GATE, t, hist=hist, pred_index=2)
    assert L.last_kernel() == "calib_hist_kernel" and L.prev_kernel() == _pixel(kind)
    assert hist2 is hist and torch.equal(hist, want_hist) and torch.equal(pred2, want_pred) and torch.equal(loss2, loss0)
    assert torch.equal(hist[2], utils.confusion_hist_device(t, pred, K)[0])
    _, _, hist3 = m.seen_gate_predict(x, EMB, UNSEEN, taus, GATE, t)
    assert torch.equal(hist3, want_hist)
    # (how far the gate moves this untrained model's group decision against the hard cut at the same tau: printed, not a property)
    moved = ((eff > float(taus[2])) != (margin > float(taus[2]))).float().mean().item()
    print("%s: the gate changes the group of %.1f%% of the pixels at tau = %g" % (kind, 100 * moved, taus[2]))
    # no target and no pred_index: embed_predict's own prediction; the mse loss rides along
    l4, p4, h4 = m.seen_gate_predict(x, EMB, UNSEEN, taus, GATE)
    assert l4 is None and h4 is None and torch.equal(p4, m.embed_predict(x, EMB)[1])
    lm, pm, _ = m.seen_gate_predict(x, EMB, UNSEEN, taus, GATE, t, pred_index=2, loss="mse")
    assert torch.equal(lm, m.szn_predict_mse(x, EMB, UNSEEN, t)[0]) and torch.equal(pm, pred)
    for bad in (dict(), dict(weight=-1.0), dict(weight=1.0, temperature=0.0), None):
        with pytest.raises(L.SznError):
            m.seen_gate_predict(x, EMB, UNSEEN, taus, bad, t)
    with pytest.raises(L.SznError):
        m.seen_gate_predict(x, EMB, [], taus, GATE, t)


def _trainer(tmp, kind="fcn32s", **kw):
    m = KINDS[kind](E).load_synthetic(1337, device=torch.device("cuda"))
    ds = SyntheticSegmentation(split="val", n_images=2, size=(H, W), n_class=K, embed_dim=E, seed=5)
    loader = torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False)
    layers = models.opt_layers(m)
    opt = optim.FusedAdam([{"params": [getattr(m, n).weight for n in layers]},
                           {"params": [getattr(m, n).bias for n in layers], "lr": 2e-5}], lr=1e-5)
    args = dict(cuda=True, model=m, optimizer=opt, train_loader=loader, val_loader=loader, log_dir=str(tmp), dataset="context",
                max_epoch=1, tb_writer=None, pixel_embeddings=E, loss_func="cos", unseen=UNSEEN, val_unseen=VAL_UNSEEN)
    args.update(kw)
    return m, loader, trainer_fcn.Trainer(**args)


def _rows(tmp, fname):
    lines = open(os.path.join(str(tmp), fname)).read().strip().split("\n")
    return lines[0].split(","), [ln.split(",") for ln in lines[1:]]


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_trainer(fast_tmp, kind):
    tmp = pathlib.Path(fast_tmp)
    # without the keyword the launch sequence of validate(True) is the plain route's, and with a threshold the sweep head's
    _, loader, t0 = _trainer(tmp / "plain", kind)
    assert t0.seen_gate is None
    t0.validate(True)
    assert (L.last_kernel(), L.prev_kernel()) == ("hist_kernel", "fh_finalize_kernel")
    data, target = next(iter(loader))
    t0._predict_device(data, target, True)
    assert (L.last_kernel(), L.prev_kernel()) == ("fh_finalize_kernel", "fh_cell_kernel")
    _, _, t1 = _trainer(tmp / "zero", kind, seen_threshold=0.0)
    t1.validate(True)
    assert (L.last_kernel(), L.prev_kernel()) == ("hist_kernel", _pixel(kind, False))
    t1._predict_device(data, target, True)
    assert (L.last_kernel(), L.prev_kernel()) == (_pixel(kind, False), "smh_margin_kernel")
    # the gate alone: the gate head at tau = 0, no sweep log of either name
    _, _, t2 = _trainer(tmp / "gate", kind, seen_gate=GATE)
    assert t2.seen_gate == dict(weight=1.0, temperature=float(np.float32(0.1)))
    t2.validate(True)
    assert (L.last_kernel(), L.prev_kernel()) == ("hist_kernel", _pixel(kind))
    assert not os.path.exists(str(tmp / "gate" / "seen_gate_log.csv")) and not os.path.exists(str(tmp / "gate" / "seen_sweep_log.csv"))
    # with a sweep: one seen_gate_log.csv row per tau, weight and temperature named, the best tau noted; seen_sweep_log.csv stays absent
    taus = np.linspace(-1.0, 1.0, 5).astype(np.float32)
    _, loader3, t3 = _trainer(tmp / "sweep", kind, seen_gate=GATE, seen_sweep=taus, seen_threshold=0.5)
    t3.validate(True)
    assert not os.path.exists(str(tmp / "sweep" / "seen_sweep_log.csv"))
    hdr, rows = _rows(tmp / "sweep", "seen_gate_log.csv")
    assert hdr == ["epoch", "iteration", "tau", "val/pxl_acc", "val/mean_iu", "val/seen/mean_iu", "val/unseen/mean_iu",
                   "val/harmonic_mean_iu", "weight", "temperature"]
    assert [float(r[2]) for r in rows] == [float(v) for v in taus]
    assert all(float(r[8]) == 1.0 and float(r[9]) == float(np.float32(0.1)) for r in rows)
    # the rows are the metrics of direct heads.soft_gate histograms accumulated over the loader
    m = t3.model
    m.eval()
    hist = torch.zeros(len(taus), K, K, dtype=torch.int64, device="cuda")
    for d, tg in loader3:
        d, lbl, _ = t3._unpack(d, tg)
        ctx, stride, fmap = m._head_map(d)
        margin = heads.seenmask_margin(ctx.coarse, E, m._engine._images["up.w"], H, W)
        heads.soft_gate(stride, fmap.float(), t3.embeddings, H, W, UNSEEN, margin, taus, 0.1, 1.0, lbl, hist=hist)
    hm = []
    for g, r in enumerate(rows):
        ma, ms, mu = utils.calib_rows(hist[g].cpu().numpy(), K, VAL_UNSEEN)
        want = [ma[0], ma[2], ms[2], mu[2], utils.harmonic_mean_iu(ms, mu)]
        got = [float(v) for v in r[3:8]]
        assert all(a == b or (a != a and b != b) for a, b in zip(got, want)), (g, got, want)
        hm.append(got[4])
    hm = np.array(hm)
    if np.isfinite(hm).any():
        best = max((i for i in range(len(hm)) if hm[i] == hm[i]), key=lambda i: (hm[i], -abs(float(taus[i]))))
        assert t3.best_seen_tau == float(taus[best]) and t3.best_seen_harmonic_mean_iu == hm[best]


def test_refused_combinations():
    m, loader, t = _trainer("/nonexistent-unused", rank=1)                 # (only rank 0 creates its log directory)
    base = dict(cuda=True, model=m, optimizer=t.optim, train_loader=loader, val_loader=loader, log_dir=t.log_dir, dataset="context",
                max_epoch=1, tb_writer=None, pixel_embeddings=E, loss_func="cos", unseen=UNSEEN, val_unseen=VAL_UNSEEN, rank=1)
    trainer_fcn.Trainer(**dict(base, seen_gate=GATE, seen_threshold=0.5, seen_sweep=[-1.0, 0.0, 1.0]))
    for over in (dict(unseen=[], val_unseen=[]), dict(pixel_embeddings=None, loss_func="cross_entropy"), dict(forced_unseen=True),
                 dict(eval_scales=(0.5, 1.0)), dict(eval_flip=True)):
        with pytest.raises(L.SznError):
            trainer_fcn.Trainer(**dict(base, **over, seen_gate=GATE))
    for bad in (dict(), dict(weight=-1.0), dict(weight=1.0, temperature=0.0), dict(weight=float("nan"))):
        with pytest.raises(L.SznError):
            trainer_fcn.Trainer(**dict(base, seen_gate=bad))
    with pytest.raises(L.SznError):
        trainer_fcn.Trainer(**dict(base, seen_gate=GATE)).validate(False)  # the plain validation has no seen-mask decision to gate
