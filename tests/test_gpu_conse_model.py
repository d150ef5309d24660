"""GPU: ConSE through the model surface (FCN32s / FCN8s .conse_predict), the trainer (conse=, conse_sweep=) and the CLI (--conse,
--conse-sweep), on the tiny synthetic set of the other trainer tests (33 x 47 images) with the softmax network's 21 classes and the
20-wide pascal class embeddings."""
import functools
import glob
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers_conse as HX  # noqa: E402
from zeroshotsemanticsegmentation_amd import _lib as L  # noqa: E402
from zeroshotsemanticsegmentation_amd import heads, models, optim, synth, trainer_fcn, utils  # noqa: E402
from zeroshotsemanticsegmentation_amd.synthetic_dataset import SyntheticSegmentation  # noqa: E402

E, K, B, H, W, T = 20, 21, 2, 33, 47, 5
# (classes 3 and 15 cover about 950 pixels each of the four validation images, as do the seen classes 7 and 9)
UNSEEN = [1, 3, 13, 15]
VAL_UNSEEN = [3, 15]
EMB = np.load(os.path.join(ROOT, "tests", "golden", "embeddings_pascal_20.npy"))
SWEEP = np.linspace(-0.25, 0.25, 5).astype(np.float32)
KINDS = {"fcn32s": models.FCN32s, "fcn8s": models.FCN8s}
PRECISIONS = {"fp32": torch.float32, "bf16": torch.bfloat16}


@functools.lru_cache(maxsize=None)
def batch():
    x = torch.from_numpy(synth.make_images(B, H, W, seed=31)).cuda()
    t = synth.make_labels(B, H, W, K, seed=32, block=8)
    t[:, :2, :3] = -1
    return x, torch.from_numpy(t).cuda()


@pytest.mark.parametrize("precision", sorted(PRECISIONS))
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_conse_predict(kind, precision):
    m = KINDS[kind](K).load_synthetic(1337, device=torch.device("cuda")).eval()
    m.set_precision(PRECISIONS[precision])
    x, t = batch()
    loss0, pred0 = m.softmax_predict(x, t)
    loss0, pred0 = loss0.clone(), pred0.clone()
    emb = torch.from_numpy(EMB).cuda()
    # the loss is softmax_predict's bit for bit; pred and hist are heads.conse's on the model's own map
    loss, pred, hist = m.conse_predict(x, EMB, UNSEEN, T, SWEEP, t, pred_index=2)
    assert L.last_kernel() == "calib_hist_kernel" and L.prev_kernel() == "conse_cell_kernel"
    assert torch.equal(loss, loss0) and loss.dim() == 0 and m._last_pred is pred
    assert hist.dtype == torch.int64 and tuple(hist.shape) == (5, K, K)
    with torch.no_grad():
        ctx, stride, fmap = m._head_map(x)
        fmap = fmap.to(torch.float32).clone()
    assert stride == (32 if kind == "fcn32s" else 8)
    want_hist, want_pred = heads.conse(stride, fmap, emb, H, W, UNSEEN, T, SWEEP, t, pred_index=2)
    assert torch.equal(pred, want_pred) and torch.equal(hist, want_hist)
    assert torch.equal(hist[2], utils.confusion_hist_device(t, pred, K)[0])
    # hist accumulates in place; no target: no loss, no histogram; every gamma's prediction has its counts in hist
    loss2, pred2, hist2 = m.conse_predict(x, EMB, UNSEEN, T, SWEEP, t, hist=hist, pred_index=4)
    assert hist2 is hist and torch.equal(loss2, loss0)
    assert torch.equal(hist[4], 2 * utils.confusion_hist_device(t, pred2, K)[0])
    l3, p3, h3 = m.conse_predict(x, EMB, UNSEEN, T, [0.25], pred_index=0)
    assert l3 is None and h3 is None and torch.equal(p3, pred2)
    _, pred_lo, _ = m.conse_predict(x, EMB, UNSEEN, T, SWEEP, pred_index=0)
    unseen = torch.tensor(UNSEEN, device="cuda")
    n_lo, n_0, n_hi = (int(torch.isin(p, unseen).sum()) for p in (pred_lo, pred, pred2))
    print("%s %s: pixels predicted unseen at gamma -0.25 / 0 / 0.25: %d / %d / %d" % (kind, precision, n_lo, n_0, n_hi))
    assert n_lo <= n_0 <= n_hi and n_lo < n_hi
    # forced: the far gammas by the target
    lf, pf, hf = m.conse_predict(x, EMB, UNSEEN, T, target=t, forced=True)
    assert torch.equal(lf, loss0) and hf is None
    _, p_a, _ = m.conse_predict(x, EMB, UNSEEN, T, [-4.0], pred_index=0)
    _, p_b, _ = m.conse_predict(x, EMB, UNSEEN, T, [4.0], pred_index=0)
    assert torch.equal(pf, torch.where(torch.isin(t, unseen), p_b, p_a))
    # the torch-op referee on the materialised score and the float64 restatement on the map agree with it on the clear pixels
    with torch.no_grad():
        score = m(x, mode="fcn").float()
    ref = HX.reference(stride, H, W, fmap[..., :K].cpu().numpy(), EMB, UNSEEN, T, SWEEP)
    clear = ~ref["unclear"][2]
    print("%s %s: %.2f %% of the pixels unclear at gamma 0" % (kind, precision, 100 * (1 - clear.mean())))
    assert clear.mean() > 0.5
    assert np.array_equal(pred.cpu().numpy()[clear], ref["pred"][2][clear])
    assert np.array_equal(utils.conse_infer(score, EMB, UNSEEN, T, 0.0).cpu().numpy()[clear], ref["pred"][2][clear])
    got_f = utils.conse_infer(score, EMB, UNSEEN, T, target=t).cpu().numpy()
    assert np.array_equal(got_f[~ref["shaky"]], pf.cpu().numpy()[~ref["shaky"]])
    for bad in (dict(unseen=[]), dict(top_t=0), dict(top_t=17), dict(gammas=[0.1, 0.0]), dict(pred_index=5), dict(forced=True)):
        kw = dict(dict(unseen=UNSEEN, top_t=T, gammas=SWEEP, target=t, pred_index=None, forced=False), **bad)
        with pytest.raises(L.SznError):
            m.conse_predict(x, EMB, **kw)
    with pytest.raises(L.SznError):
        m.conse_predict(x, EMB[:20], UNSEEN, T, SWEEP, t)


def _trainer(tmp, kind="fcn32s", **kw):
    m = KINDS[kind](K).load_synthetic(1337, device=torch.device("cuda"))
    ds = SyntheticSegmentation(split="val", n_images=4, size=(H, W), n_class=K, embed_dim=0, seed=5)
    loader = torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False)
    layers = models.opt_layers(m)
    opt = optim.FusedSGD([{"params": [getattr(m, n).weight for n in layers]},
                          {"params": [getattr(m, n).bias for n in layers], "lr": 2e-10}], lr=1e-10, momentum=0.99)
    args = dict(cuda=True, model=m, optimizer=opt, train_loader=loader, val_loader=loader, log_dir=str(tmp), dataset="pascal",
                max_epoch=1, tb_writer=None, pixel_embeddings=0, loss_func="cross_entropy", unseen=UNSEEN, val_unseen=VAL_UNSEEN,
                embed_arr=EMB)
    args.update(kw)
    return m, loader, trainer_fcn.Trainer(**args)


def _rows(tmp, fname):
    lines = open(os.path.join(str(tmp), fname)).read().strip().split("\n")
    return lines[0].split(","), [ln.split(",") for ln in lines[1:]]


def _val_numbers(tmp):
    hdr, rows = _rows(tmp, "val_log.csv")
    assert len(rows) == 1
    return {k: float(v) for k, v in zip(hdr[2:-1], rows[0][2:-1])}        # (without epoch, iteration and the elapsed time)


def _kernels(trainer, loader):
    """the kernels one validation batch launches last"""
    data, target = next(iter(loader))
    trainer.model.eval()
    with torch.no_grad():
        trainer._predict_device(data, target, False)
    return L.prev_kernel(), L.last_kernel()


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_trainer(kind, fast_tmp):
    tmp = pathlib.Path(fast_tmp)                 # validate() writes a full checkpoint per call
    _, loader0, t0 = _trainer(tmp / "plain", kind)
    assert t0.conse is None and t0.conse_sweep is None
    t0.validate()
    plain = _val_numbers(tmp / "plain")
    assert not os.path.exists(str(tmp / "plain" / "conse_log.csv"))
    assert _kernels(t0, loader0)[1] == "ce_finalize_kernel"      # a trainer without conse launches what it did before
    # conse with a sweep: val_log from the ConSE prediction at gamma, conse_log one row per gamma
    m1, loader, t1 = _trainer(tmp / "conse", kind, conse=dict(top=T, dim=E, gamma=0.125), conse_sweep=SWEEP)
    assert t1.conse == dict(top=T, dim=E, gamma=0.125)
    t1.validate()
    got = _val_numbers(tmp / "conse")
    assert got["val/loss"] == plain["val/loss"]
    assert _kernels(t1, loader) == ("conse_cell_kernel", "calib_hist_kernel")
    hdr, rows = _rows(tmp / "conse", "conse_log.csv")
    assert hdr == ["epoch", "iteration", "gamma", "val/pxl_acc", "val/mean_iu", "val/seen/mean_iu", "val/unseen/mean_iu",
                   "val/harmonic_mean_iu"]
    assert [float(r[2]) for r in rows] == [float(g) for g in SWEEP]
    hm = np.array([float(r[7]) for r in rows])
    assert np.isfinite(hm).all()
    for r, h in zip(rows, hm):
        s, u = float(r[5]), float(r[6])
        assert h == (2 * s * u / (s + u) if s + u else 0.0)
    best = max(range(len(hm)), key=lambda i: (hm[i], -abs(float(SWEEP[i]))))
    assert t1.best_conse_gamma == float(SWEEP[best]) and t1.best_conse_harmonic_mean_iu == hm[best] == hm.max()
    # val_log against the referee on the materialised score: the two may differ on unclear pixels only, so the numbers are checked
    # against the fused prediction's own counts exactly, and the fused prediction against the referee pixel by pixel
    emb = torch.from_numpy(EMB).cuda()
    hist = torch.zeros(1, K, K, dtype=torch.int64, device="cuda")
    m1.eval()
    differ = total = 0
    for data, target in loader:
        data, lbl, _ = t1._unpack(data, target)
        _, pred, _ = m1.conse_predict(data, emb, UNSEEN, T, [0.125], lbl, hist=hist, pred_index=0)
        with torch.no_grad():
            ctx, stride, fmap = m1._head_map(data)
            fmap = fmap.to(torch.float32)[..., :K].cpu().numpy()
            score = m1(data, mode="fcn").float()
        ref = HX.reference(stride, H, W, fmap, EMB, UNSEEN, T, [np.float32(0.125)])
        clear = ~ref["unclear"][0]
        want = utils.conse_infer(score, emb, UNSEEN, T, 0.125).cpu().numpy()
        assert np.array_equal(pred.cpu().numpy()[clear], want[clear])
        differ += int((pred.cpu().numpy() != want).sum())
        total += want.size
    print("%s: fused and referee differ on %d of %d pixels (all unclear)" % (kind, differ, total))
    want = utils.calib_rows(hist[0].cpu().numpy(), K, VAL_UNSEEN)
    assert got["val/mean_iu"] == want[0][2] and got["val/seen/mean_iu"] == want[1][2] and got["val/unseen/mean_iu"] == want[2][2]
    # forced unseen: the unseen rows come from the unseen classes alone
    _, _, t2 = _trainer(tmp / "forced", kind, conse=dict(top=T, dim=E), forced_unseen=True)
    t2.validate()
    assert _val_numbers(tmp / "forced")["val/unseen/mean_iu"] >= 0.0
    assert not os.path.exists(str(tmp / "forced" / "conse_log.csv"))


def test_refused_combinations():
    m, loader, t = _trainer("/nonexistent-unused", rank=1)                 # (only rank 0 creates its log directory)
    base = dict(cuda=True, model=m, optimizer=t.optim, train_loader=loader, val_loader=loader, log_dir=t.log_dir, dataset="pascal",
                max_epoch=1, tb_writer=None, pixel_embeddings=0, loss_func="cross_entropy", unseen=UNSEEN, val_unseen=VAL_UNSEEN, rank=1,
                embed_arr=EMB)
    ok = dict(conse=dict(top=T, dim=E, gamma=0.1), conse_sweep=SWEEP)
    trainer_fcn.Trainer(**dict(base, **ok))
    trainer_fcn.Trainer(**dict(base, conse=dict(top=T), forced_unseen=True))
    bad = [dict(unseen=[], val_unseen=[]), dict(loss_func="cos"), dict(eval_scales=(0.5, 1.0)), dict(eval_flip=True),
           dict(forced_unseen=True), dict(embed_arr=EMB[:20])]
    for over in bad:
        with pytest.raises(L.SznError):
            trainer_fcn.Trainer(**dict(base, **ok, **over))
    for cfg in (dict(conse=dict(top=0)), dict(conse=dict(top=17)), dict(conse=dict(dim=E)), dict(conse=dict(top=T, gamma=float("nan"))),
                dict(conse=dict(top=T, tau=1.0)), dict(conse_sweep=SWEEP), dict(conse=dict(top=T), conse_sweep=[0.1, 0.0])):
        with pytest.raises(L.SznError):
            trainer_fcn.Trainer(**dict(base, **cfg))
    # -m test_all (the seen-mask-stitched validation) is out of scope
    tc = trainer_fcn.Trainer(**dict(base, conse=dict(top=T)))
    with pytest.raises(L.SznError):
        tc.validate(both_fcn_and_seenmask=True)


def test_cli_conse_sweep_in_a_child_process(fast_tmp):
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "-c", "1", "-tu", "1,13", "-vu", "17,19", "--synthetic", "16", "64", "64",
           "--conse", "5", "--conse-sweep", "-0.5", "0.5", "17", "-ve", "1", "-dir", fast_tmp, "-n", "conse", "--workers", "0"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    log = glob.glob(os.path.join(fast_tmp, "logs", "conse_CFG_1_*"))[0]
    hdr, rows = _rows(log, "conse_log.csv")
    assert len(rows) == 17 and float(rows[0][2]) == -0.5 and float(rows[8][2]) == 0.0 and float(rows[16][2]) == 0.5
    assert "conse: " in r.stdout
