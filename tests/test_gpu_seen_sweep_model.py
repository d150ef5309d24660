"""GPU: the seen-mask threshold through the model surface (FCN32s / FCN8s .seen_sweep_predict), the trainer (seen_threshold=,
seen_sweep=, validate(True)) and the CLI (-m test_all --seen-sweep), on the tiny synthetic set of the other trainer tests (33 x 47
images, 33 classes, E = 20)."""
import functools
import glob
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
from zeroshotsemanticsegmentation_amd import heads, models, optim, synth, train, trainer_fcn, utils  # noqa: E402
from zeroshotsemanticsegmentation_amd.synthetic_dataset import SyntheticSegmentation  # noqa: E402

E, K, B, H, W = 20, 33, 2, 33, 47
# (classes 15 and 24 cover about 1000 pixels each of the four validation images)
UNSEEN = [0, 12, 15, 24]
VAL_UNSEEN = [15, 24]
EMB = np.load(os.path.join(ROOT, "tests", "golden", "embeddings_context_20.npy"))
KINDS = {"fcn32s": models.FCN32s, "fcn8s": models.FCN8s}


@functools.lru_cache(maxsize=None)
def net(kind):
    return KINDS[kind](E).load_synthetic(1337, device=torch.device("cuda")).eval()


@functools.lru_cache(maxsize=None)
def batch():
    x = torch.from_numpy(synth.make_images(B, H, W, seed=31)).cuda()
    t = synth.make_labels(B, H, W, K, seed=32, block=8)
    t[:, :2, :3] = -1
    return x, torch.from_numpy(t).cuda()


def _sweep_for(margin, n=5):
    """n ascending taus spread over the margins the model gives, 0 among them"""
    lo, hi = float(margin.min()), float(margin.max())
    assert lo < 0 < hi, "the synthetic seen-mask head decides both ways"
    return np.unique(np.concatenate([np.linspace(lo / 2, hi / 2, n - 1), [0.0]]).astype(np.float32))


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_seen_sweep_predict(kind):
    m = net(kind)
    x, t = batch()
    loss0, pred0 = m.szn_predict(x, EMB, UNSEEN, t)
    pred0, group0 = pred0.clone(), m._last_group.clone()
    # taus = [0]: szn_predict's loss and prediction, bit for bit
    pixel = "sweep_cell_kernel" if kind == "fcn32s" else "sweep_cell_tab_kernel"
    loss, pred, hist = m.seen_sweep_predict(x, EMB, UNSEEN, [0.0], t, pred_index=0)
    # (a prediction-only call: no histogram asked for, no crossing tables, no histogram kernel)
    assert hist is None and L.last_kernel() == pixel and L.prev_kernel() == "smh_margin_kernel" and m._last_pred is pred
    _, _, hist = m.seen_sweep_predict(x, EMB, UNSEEN, [0.0], t)
    assert L.last_kernel() == "calib_hist_kernel" and L.prev_kernel() == pixel
    assert torch.equal(loss, loss0) and loss.dim() == 0 and torch.equal(pred, pred0)
    margin = m._last_margin.clone()
    assert margin.dtype == torch.float32 and tuple(margin.shape) == (B, H, W) and torch.equal((margin > 0).long(), group0)
    assert tuple(hist.shape) == (1, K, K) and torch.equal(hist[0], utils.confusion_hist_device(t, pred0, K)[0])
    # a sweep: every tau's histogram is that of the grouped head on the thresholded margin; hist accumulates in place
    taus = _sweep_for(margin)
    z = int(np.flatnonzero(taus == 0)[0])
    hist = torch.zeros(len(taus), K, K, dtype=torch.int64, device="cuda")
    loss2, pred_z, hist2 = m.seen_sweep_predict(x, EMB, UNSEEN, taus, t, hist=hist, pred_index=z)
    assert hist2 is hist and torch.equal(loss2, loss0) and torch.equal(pred_z, pred0)
    _, stride, fmap = m._head_map(x)
    fmap = fmap.float().clone()                      # (the next forward pass reuses the engine's buffers)
    emb = torch.from_numpy(EMB).cuda()
    n_unseen = []
    for g, tau in enumerate(taus):
        want = heads.embed_predict("cos", stride, fmap, emb, H, W, None, 1, UNSEEN, (margin > float(tau)).long())[1]
        _, pg, _ = m.seen_sweep_predict(x, EMB, UNSEEN, taus, pred_index=g)
        assert torch.equal(pg, want), g
        assert torch.equal(hist[g], utils.confusion_hist_device(t, want, K)[0]), g
        n_unseen.append(int((margin > float(tau)).logical_not().sum()))
    print("%s: pixels in the unseen group per tau %s: %s" % (kind, taus.tolist(), n_unseen))
    assert (np.diff(n_unseen) >= 0).all() and n_unseen[0] < n_unseen[-1]
    _, _, hist_b = m.seen_sweep_predict(x, EMB, UNSEEN, taus, t, hist=hist.clone())
    assert torch.equal(hist_b, 2 * hist)
    # pred_index None: embed_predict's own prediction; no target and no pred_index: nothing but it
    l3, p3, h3 = m.seen_sweep_predict(x, EMB, UNSEEN, taus)
    assert l3 is None and h3 is None and torch.equal(p3, m.embed_predict(x, EMB)[1])
    # the mse loss rides along like in szn_predict_mse
    lm, pm, _ = m.seen_sweep_predict(x, EMB, UNSEEN, [0.0], t, pred_index=0, loss="mse")
    assert torch.equal(lm, m.szn_predict_mse(x, EMB, UNSEEN, t)[0]) and torch.equal(pm, pred0)
    with pytest.raises(L.SznError):
        m.seen_sweep_predict(x, EMB, [], taus, t)
    with pytest.raises(L.SznError):
        m.seen_sweep_predict(x, EMB, UNSEEN, [0.1, 0.0], t)
    with pytest.raises(L.SznError):
        m.seen_sweep_predict(x, EMB, UNSEEN, taus, t, pred_index=len(taus))


def _trainer(tmp, kind="fcn32s", **kw):
    m = KINDS[kind](E).load_synthetic(1337, device=torch.device("cuda"))
    ds = SyntheticSegmentation(split="val", n_images=4, size=(H, W), n_class=K, embed_dim=E, seed=5)
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


def _val_numbers(tmp):
    hdr, rows = _rows(tmp, "val_log.csv")
    assert len(rows) == 1
    return {k: float(v) for k, v in zip(hdr[2:-1], rows[0][2:-1])}        # (without epoch, iteration and the elapsed time)


def _same(a, b):
    return a.keys() == b.keys() and all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in a)


def _model_taus(t, loader):
    """a 5-tau sweep spread over the margins the trainer's model gives on the validation images (0 among the taus)"""
    lo, hi = [], []
    for data, target in loader:
        data = t._unpack(data, target)[0]
        t.model.seen_sweep_predict(data, t.embeddings, UNSEEN, [0.0], pred_index=0)
        lo.append(float(t.model._last_margin.min()))
        hi.append(float(t.model._last_margin.max()))
    lo, hi = min(lo), max(hi)
    assert lo < 0 < hi
    return np.unique(np.concatenate([np.linspace(lo / 2, hi / 2, 4), [0.0]]).astype(np.float32))


def _check_sweep(tmp, t, taus, loader):
    """seen_sweep_log.csv against metrics recomputed from per-tau szn_predict-style runs: seenmask margin thresholded in torch, the grouped
    head, szn_confusion_hist_k"""
    hdr, rows = _rows(tmp, "seen_sweep_log.csv")
    assert hdr == ["epoch", "iteration", "tau", "val/pxl_acc", "val/mean_iu", "val/seen/mean_iu", "val/unseen/mean_iu",
                   "val/harmonic_mean_iu"]
    assert [float(r[2]) for r in rows] == [float(v) for v in taus]
    m = t.model
    m.eval()
    hist = torch.zeros(len(taus), K, K, dtype=torch.int64, device="cuda")
    for data, target in loader:
        data, lbl, _ = t._unpack(data, target)
        ctx, stride, fmap = m._head_map(data)
        margin = heads.seenmask_margin(ctx.coarse, E, m._engine._images["up.w"], H, W)
        for g, tau in enumerate(taus):
            pred = heads.embed_predict("cos", stride, fmap, t.embeddings, H, W, None, 1, UNSEEN, (margin > float(tau)).long())[1]
            hist[g] += utils.confusion_hist_device(lbl, pred, K)[0]
    hm = []
    for g, r in enumerate(rows):
        ma, ms, mu = utils.calib_rows(hist[g].cpu().numpy(), K, VAL_UNSEEN)
        want = [ma[0], ma[2], ms[2], mu[2], utils.harmonic_mean_iu(ms, mu)]
        got = [float(v) for v in r[3:]]
        assert all(a == b or (a != a and b != b) for a, b in zip(got, want)), (g, got, want)
        hm.append(got[4])
    hm = np.array(hm)
    if np.isfinite(hm).any():
        best = max((i for i in range(len(hm)) if hm[i] == hm[i]), key=lambda i: (hm[i], -abs(float(taus[i]))))
        assert t.best_seen_tau == float(taus[best]) and t.best_seen_harmonic_mean_iu == hm[best]
    return rows


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_trainer(fast_tmp, kind):
    tmp = pathlib.Path(fast_tmp)                 # validate() writes a full checkpoint per call
    pixel = "sweep_cell_kernel" if kind == "fcn32s" else "sweep_cell_tab_kernel"
    _, loader, t0 = _trainer(tmp / "plain", kind)
    assert t0.seen_threshold is None and t0.seen_sweep is None
    t0.validate(True)
    plain = _val_numbers(tmp / "plain")
    assert not os.path.exists(str(tmp / "plain" / "seen_sweep_log.csv"))
    data, target = next(iter(loader))
    # without the keywords the route is szn_predict's: the seen-mask head, then the grouped head (which notes its pixel kernel as
    # fh_cell_kernel at either stride)
    x0, lbl0, _ = t0._unpack(data, target)
    assert (L.last_kernel(), L.prev_kernel()) == ("hist_kernel", "fh_finalize_kernel")      # after validate(True): szn_confusion_hist_k
    t0.model.szn_predict(x0, t0.embeddings, UNSEEN, lbl0)
    assert (L.last_kernel(), L.prev_kernel()) == ("fh_finalize_kernel", "fh_cell_kernel")
    t0._predict_device(data, target, True)
    assert (L.last_kernel(), L.prev_kernel()) == ("fh_finalize_kernel", "fh_cell_kernel")
    # seen_threshold = 0: the same numbers, on the sweep head
    _, _, t1 = _trainer(tmp / "zero", kind, seen_threshold=0.0)
    t1.validate(True)
    assert (L.last_kernel(), L.prev_kernel()) == ("hist_kernel", pixel)
    assert _same(_val_numbers(tmp / "zero"), plain)
    assert not os.path.exists(str(tmp / "zero" / "seen_sweep_log.csv"))
    t1._predict_device(data, target, True)
    assert (L.last_kernel(), L.prev_kernel()) == (pixel, "smh_margin_kernel")           # prediction only: no histogram kernel
    # a sweep alone: val_log unchanged (the reported prediction stays tau = 0's), one seen_sweep_log row per tau
    taus = _model_taus(t0, loader)
    _, loader2, t2 = _trainer(tmp / "sweep", kind, seen_sweep=taus)
    t2.validate(True)
    assert _same(_val_numbers(tmp / "sweep"), plain)
    rows = _check_sweep(tmp / "sweep", t2, taus, loader2)
    z = int(np.flatnonzero(taus == 0)[0])
    hdr = _rows(tmp / "sweep", "seen_sweep_log.csv")[0]
    zero = {k: float(v) for k, v in zip(hdr, rows[z])}
    for k in ("val/pxl_acc", "val/mean_iu", "val/seen/mean_iu", "val/unseen/mean_iu"):
        assert zero[k] == plain[k] or (zero[k] != zero[k] and plain[k] != plain[k]), k       # exactly: the same integer counts
    # a threshold that is not one of the sweep's taus, a sweep without 0: val_log is that threshold's, the log still the sweep's
    other = taus[taus != 0]
    tau_x = float(np.float32((other[-1] + other[-2]) / 2))
    _, loader3, t3 = _trainer(tmp / "both", kind, seen_threshold=tau_x, seen_sweep=other)
    t3.validate(True)
    rows3 = _check_sweep(tmp / "both", t3, other, loader3)
    assert [r[2:] for r in rows3] == [r[2:] for r in rows if float(r[2]) != 0.0]
    _, loader4, t4 = _trainer(tmp / "thr", kind, seen_threshold=tau_x)
    t4.validate(True)
    assert _same(_val_numbers(tmp / "thr"), _val_numbers(tmp / "both"))


def test_refused_combinations():
    m, loader, t = _trainer("/nonexistent-unused", rank=1)                 # (only rank 0 creates its log directory)
    base = dict(cuda=True, model=m, optimizer=t.optim, train_loader=loader, val_loader=loader, log_dir=t.log_dir, dataset="context",
                max_epoch=1, tb_writer=None, pixel_embeddings=E, loss_func="cos", unseen=UNSEEN, val_unseen=VAL_UNSEEN, rank=1)
    trainer_fcn.Trainer(**dict(base, seen_threshold=0.5, seen_sweep=[-1.0, 0.0, 1.0]))
    bad = [dict(unseen=[], val_unseen=[]), dict(pixel_embeddings=None, loss_func="cross_entropy"), dict(forced_unseen=True),
           dict(eval_scales=(0.5, 1.0)), dict(eval_flip=True)]
    for over in bad:
        for kw in (dict(seen_threshold=0.5), dict(seen_sweep=[-1.0, 1.0])):
            with pytest.raises(L.SznError):
                trainer_fcn.Trainer(**dict(base, **over, **kw))
    for kw in (dict(seen_threshold=float("nan")), dict(seen_sweep=[0.1, 0.0]), dict(seen_sweep=np.arange(65))):
        with pytest.raises(L.SznError):
            trainer_fcn.Trainer(**dict(base, **kw))
    # the plain validation (and with it train()) has no seen-mask decision to threshold
    for kw in (dict(seen_threshold=0.5), dict(seen_sweep=[-1.0, 1.0])):
        with pytest.raises(L.SznError):
            trainer_fcn.Trainer(**dict(base, **kw)).validate(False)
    # a 64-tau sweep without 0 has no room for the reported threshold
    with pytest.raises(L.SznError):
        trainer_fcn.Trainer(**dict(base, seen_sweep=np.arange(1, 65))).validate(True)


def test_refused_with_verbose_val(monkeypatch):
    monkeypatch.setenv("SZN_VERBOSE_VAL", "1")
    with pytest.raises(L.SznError):
        _trainer("/nonexistent-unused", seen_threshold=0.5, rank=1)


def test_cli_test_all_seen_sweep(fast_tmp, capsys):
    # a checkpoint of the synthetic model stands for a trained run (-m test_all loads <dir>/logs/<run>/best)
    run = os.path.join(fast_tmp, "logs", "ck")
    os.makedirs(run)
    torch.save({"epoch": 0, "iteration": 0, "arch": "FCN32s", "model_state_dict": models.FCN32s(E).load_synthetic(1337).state_dict(),
                "best_mean_iu": 0}, os.path.join(run, "best"))
    # (-vu 22,24: classes the synthetic validation images contain)
    common = ["--synthetic", "4", "33", "47", "-c", "18", "-vu", "22,24", "-r", "ck", "-dir", fast_tmp, "--workers", "0"]
    train.main(common + ["-m", "test_all", "--seen-sweep", "-2", "2", "5", "-n", "sw"])
    out = capsys.readouterr().out
    log = glob.glob(os.path.join(fast_tmp, "logs", "sw_CFG_18_*"))[0]
    hdr, rows = _rows(log, "seen_sweep_log.csv")
    assert hdr[2] == "tau" and len(rows) == 5 and [float(r[2]) for r in rows] == [-2.0, -1.0, 0.0, 1.0, 2.0]
    assert "seen-mask threshold: best tau" in out or "seen-mask threshold: no tau" in out
    # the flags belong to -m test_all
    with pytest.raises(Exception, match="--seen-threshold / --seen-sweep: a seen-mask threshold acts on the full SZN network only"):
        train.main(common + ["-m", "test_fcn", "--seen-threshold", "0.5", "-n", "bad"])
