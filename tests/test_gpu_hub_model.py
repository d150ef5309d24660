"""GPU: the hubness correction through the model surface (FCN32s / FCN8s .hub_predict) against the torch-op referee utils.hub_infer on
the score the same model materialises, and through the trainer (hub=, hub_log.csv), on tiny synthetic inputs (33 x 47 and 70 x 90 images,
33 classes, E = 20, fp32)."""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers_hub as HH  # noqa: E402
import helpers_msinfer as HM  # noqa: E402
from zeroshotsemanticsegmentation_amd import _lib as L  # noqa: E402
from zeroshotsemanticsegmentation_amd import heads, models, optim, synth, trainer_fcn, utils  # noqa: E402
from zeroshotsemanticsegmentation_amd.synthetic_dataset import SyntheticSegmentation  # noqa: E402

E, K = 20, 33
UNSEEN = [0, 12, 15, 24]
VAL_UNSEEN = [15, 24]
EMB = np.load(os.path.join(ROOT, "tests", "golden", "embeddings_context_20.npy"))
SWEEP = np.linspace(-0.25, 0.25, 5).astype(np.float32)
KINDS = {"fcn32s": models.FCN32s, "fcn8s": models.FCN8s}
SIZES = {"33x47": (2, 33, 47), "70x90": (1, 70, 90)}


@functools.lru_cache(maxsize=None)
def net(kind):
    return KINDS[kind](E).load_synthetic(1337, device=torch.device("cuda")).eval()


@functools.lru_cache(maxsize=None)
def batch(size):
    B, H, W = SIZES[size]
    x = torch.from_numpy(synth.make_images(B, H, W, seed=31)).cuda()
    t = synth.make_labels(B, H, W, K, seed=32, block=8)
    t[:, :2, :3] = -1
    t[:, -3:, :] = HH.PAD
    return x, torch.from_numpy(t).cuda()


def _pixel(kind):
    return "hub_cell_kernel" if kind == "fcn32s" else "hub_cell_tab_kernel"


@pytest.mark.parametrize("mode", HH.MODES)
@pytest.mark.parametrize("size", sorted(SIZES))
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_hub_predict_against_the_referee(kind, size, mode):
    m = net(kind)
    x, t = batch(size)
    B, H, W = SIZES[size]
    hub = dict(mode=mode, beta=HH.BETA, min_sd=HH.MIN_SD)
    gam = HH.gammas(mode)[6:11]                                   # five gammas around 0
    loss0, _ = m.embed_predict(x, EMB, t)
    loss, pred, hist = m.hub_predict(x, EMB, UNSEEN, hub, gam, t, pred_index=2)
    assert L.last_kernel() == "calib_hist_kernel" and L.prev_kernel() == _pixel(kind) and m._last_pred is pred
    assert torch.equal(loss, loss0) and loss.dim() == 0                      # the loss is the stored image's, unchanged
    table = m._last_hub_table.clone()
    assert tuple(table.shape) == (B, K, 2) and tuple(hist.shape) == (5, K, K)
    assert torch.equal(hist[2], utils.confusion_hist_device(t, pred, K)[0])
    # pred and hist are direct heads.hub_stats / heads.hub calls' on the kept map
    _, stride, fmap = m._head_map(x)
    fmap = fmap.detach().float().clone()             # (the next forward pass reuses the engine's buffers)
    emb = torch.from_numpy(EMB).cuda()
    tab2, counts = heads.hub_stats(stride, fmap, emb, H, W, mode, HH.BETA, HH.MIN_SD, t, want=("counts",))
    assert torch.equal(tab2, table) and (counts < H * W).all() and (counts > 0).all()
    want_hist, want_pred = heads.hub(stride, fmap, emb, H, W, UNSEEN, table, gam, t, pred_index=2)
    assert torch.equal(pred, want_pred) and torch.equal(hist, want_hist)
    # the referee on the materialised score, clear pixels only: float64 similarities from the same map, the device's table, and the
    # per-class error of tests/helpers_hub.py decide which pixels are clear
    sim, kappa = HM.view_sims(fmap[..., :E].cpu().numpy(), stride, H, W, H, W, False, EMB)
    ref = HH.reference(sim, HM.bound(1, kappa, E), UNSEEN, table.cpu().numpy(), gam)
    with torch.no_grad():
        score = m(x, mode="fcn").float()
    valid = t != HH.PAD
    clear_all = ~ref["unclear"].any(axis=0)
    for gi in range(len(gam)):
        _, p, _ = m.hub_predict(x, EMB, UNSEEN, hub, gam, t, pred_index=gi)
        referee = utils.hub_infer(score, emb, UNSEEN, mode, HH.BETA, float(gam[gi]), HH.MIN_SD, valid)
        clear = ~ref["unclear"][gi]
        assert np.array_equal(p.cpu().numpy()[clear], ref["pred"][gi][clear]), gi
        assert np.array_equal(referee.cpu().numpy()[clear], p.cpu().numpy()[clear]), gi
    print("%s %s %s: %.4f of the pixels clear at all five gammas" % (kind, size, mode, clear_all.mean()))
    assert clear_all.mean() > 0.25
    # no target and no pred_index: embed_predict's own prediction; the mse loss rides along
    l4, p4, h4 = m.hub_predict(x, EMB, UNSEEN, hub, gam)
    assert l4 is None and h4 is None and torch.equal(p4, m.embed_predict(x, EMB)[1])
    lm, pm, _ = m.hub_predict(x, EMB, UNSEEN, hub, gam, t, pred_index=2, loss="mse")
    assert torch.equal(lm, m.embed_predict(x, EMB, t, loss="mse")[0]) and torch.equal(pm, pred)
    for bad in (dict(), dict(mode="median"), dict(mode="mean", beta=-1.0), None):
        with pytest.raises(L.SznError):
            m.hub_predict(x, EMB, UNSEEN, bad, gam, t)
    with pytest.raises(L.SznError):
        m.hub_predict(x, EMB, [], hub, gam, t)


def _trainer(tmp, kind="fcn32s", **kw):
    H, W = 33, 47
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


HDR = ["epoch", "iteration", "row", "mode", "beta", "min_sd", "gamma", "val/mean_iu", "val/seen/mean_iu", "val/unseen/mean_iu",
       "val/harmonic_mean_iu", "val/hubness_skew"]


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_trainer(fast_tmp, kind):
    tmp = pathlib.Path(fast_tmp)
    # without the keyword validation launches exactly what it launched before: the plain route's kernels, and with a calibration the
    # calibrated head's -- never a hub kernel, and no hub_log.csv
    m0, loader, t0 = _trainer(tmp / "plain", kind)
    assert t0.hub is None
    data, target = next(iter(loader))
    d0, lbl0, _ = t0._unpack(data, target)
    m0.eval()
    m0.embed_predict(d0, t0.embeddings, lbl0)
    plain_names = (L.last_kernel(), L.prev_kernel())
    t0._predict_device(data, target, False)
    assert (L.last_kernel(), L.prev_kernel()) == plain_names and not any("hub" in n or "calib" in n for n in plain_names)
    t0.validate()
    assert L.last_kernel() == "hist_kernel" and L.prev_kernel() == plain_names[0]
    _, _, t1 = _trainer(tmp / "cal", kind, calibration=0.0, calib_sweep=SWEEP)
    t1._predict_device(data, target, False)
    assert (L.last_kernel(), L.prev_kernel()) == ("calib_hist_kernel", _pixel(kind).replace("hub", "calib"))
    t1.validate()
    for d in ("plain", "cal"):
        assert not os.path.exists(str(tmp / d / "hub_log.csv"))
    assert os.path.exists(str(tmp / "cal" / "calib_log.csv"))
    # the correction alone: the hub head at gamma 0, one 'used' row, no calib_log.csv
    hub = dict(mode="mean", beta=1.0, min_sd=0.05)
    _, _, t2 = _trainer(tmp / "hub", kind, hub=dict(mode="mean"))
    assert t2.hub == dict(mode="mean", beta=1.0, min_sd=float(np.float32(0.05)))
    t2._predict_device(data, target, False)
    assert (L.last_kernel(), L.prev_kernel()) == ("calib_hist_kernel", _pixel(kind))
    t2.validate()
    assert not os.path.exists(str(tmp / "hub" / "calib_log.csv"))
    hdr, rows = _rows(tmp / "hub", "hub_log.csv")
    assert hdr == HDR and len(rows) == 1 and rows[0][2:7] == ["used", "mean", "1.0", str(float(np.float32(0.05))), "0.0"]
    assert float(rows[0][11]) == t2.last_hub_skew and np.isfinite(t2.last_hub_skew)
    # with a sweep and a calibration that is not one of its gammas: the 'used' row is that gamma's, then one 'sweep' row per gamma of the
    # sweep; calib_log.csv stays absent
    m3, loader3, t3 = _trainer(tmp / "sweep", kind, hub=dict(mode="zscore", beta=0.5), calibration=0.2, calib_sweep=SWEEP)
    t3.validate()
    assert not os.path.exists(str(tmp / "sweep" / "calib_log.csv"))
    hdr, rows = _rows(tmp / "sweep", "hub_log.csv")
    assert hdr == HDR and [r[2] for r in rows] == ["used"] + ["sweep"] * 5
    assert all(r[3] == "zscore" and float(r[4]) == 0.5 and float(r[5]) == float(np.float32(0.05)) for r in rows)
    assert [float(r[6]) for r in rows] == [float(np.float32(0.2))] + [float(g) for g in SWEEP]
    # the rows are the metrics of direct hub_predict histograms accumulated over the loader
    gam = np.unique(np.concatenate([SWEEP, np.float32([0.2])]))
    hist = torch.zeros(len(gam), K, K, dtype=torch.int64, device="cuda")
    m3.eval()
    for d, tg in loader3:
        d, lbl, _ = t3._unpack(d, tg)
        m3.hub_predict(d, t3.embeddings, UNSEEN, t3.hub, gam, lbl, hist=hist)
    hist = hist.cpu().numpy()
    hm = []
    for r in rows:
        h = hist[int(np.searchsorted(gam, np.float32(r[6])))]
        ma, ms, mu = utils.calib_rows(h, K, VAL_UNSEEN)
        want = [ma[2], ms[2], mu[2], utils.harmonic_mean_iu(ms, mu), utils.hubness_skew(h)]
        got = [float(v) for v in r[7:12]]
        assert all(a == b or (a != a and b != b) for a, b in zip(got, want)), (r[2], r[6], got, want)
        hm.append(got[3])
    hm = np.array(hm[1:])
    if np.isfinite(hm).any():
        best = max((i for i in range(len(hm)) if hm[i] == hm[i]), key=lambda i: (hm[i], -abs(float(SWEEP[i]))))
        assert t3.best_gamma == float(SWEEP[best]) and t3.best_harmonic_mean_iu == hm[best]


def test_refused_combinations():
    m, loader, t = _trainer("/nonexistent-unused", rank=1)                 # (only rank 0 creates its log directory)
    base = dict(cuda=True, model=m, optimizer=t.optim, train_loader=loader, val_loader=loader, log_dir=t.log_dir, dataset="context",
                max_epoch=1, tb_writer=None, pixel_embeddings=E, loss_func="cos", unseen=UNSEEN, val_unseen=VAL_UNSEEN, rank=1)
    hub = dict(mode="mean")
    trainer_fcn.Trainer(**dict(base, hub=hub, calibration=0.1, calib_sweep=SWEEP))
    for over in (dict(unseen=[], val_unseen=[]), dict(pixel_embeddings=None, loss_func="cross_entropy"), dict(forced_unseen=True),
                 dict(eval_scales=(0.5, 1.0)), dict(eval_flip=True)):
        with pytest.raises(L.SznError):
            trainer_fcn.Trainer(**dict(base, **over, hub=hub))
    for bad in (dict(), dict(mode="median"), dict(mode="mean", beta=-1.0), dict(mode="zscore", min_sd=0.0)):
        with pytest.raises(L.SznError):
            trainer_fcn.Trainer(**dict(base, hub=bad))
    with pytest.raises(L.SznError):
        trainer_fcn.Trainer(**dict(base, hub=hub)).validate(both_fcn_and_seenmask=True)    # -m test_all has its own class-assignment rule


def test_refused_with_verbose_val(monkeypatch):
    monkeypatch.setenv("SZN_VERBOSE_VAL", "1")
    with pytest.raises(L.SznError):
        _trainer("/nonexistent-unused", hub=dict(mode="mean"), rank=1)
