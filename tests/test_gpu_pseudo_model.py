"""GPU: self-training pseudo labels through the host layers -- engine.TrainStep(pseudo=), Trainer(pseudo=, pseudo_start_epoch=) and
train.py --pseudo-label -- on B = 2, 64 x 64, E = 20, K = 21 with three unseen classes: FCN32s and FCN8s in fp32, FCN32s in bf16.
The labelling rule runs at gamma = 2.5: a margin of two cosines never exceeds 2, so every hidden pixel is a candidate whatever the
untrained network predicts, and the selection has something to select."""
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
from zeroshotsemanticsegmentation_amd import _lib as L  # noqa: E402
from zeroshotsemanticsegmentation_amd import datasets, engine, heads, models, optim, synth, trainer_fcn, utils  # noqa: E402
from zeroshotsemanticsegmentation_amd.synthetic_dataset import SyntheticSegmentation  # noqa: E402

E, K, B, H, W = 20, 21, 2, 64, 64
UNSEEN = [2, 5, 8]
HIDDEN = datasets.HIDDEN_LABEL
CFG = dict(unseen=UNSEEN, gamma=2.5, keep=0.3, conf_floor=-2.0)
EMB = synth.make_embeddings(K, E)
KINDS = {"fcn32s": models.FCN32s, "fcn8s": models.FCN8s}


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def batch(hide=True):
    """images, and labels in 8 x 8 blocks over all classes with a -1 sprinkle, a -2 border; hide: the unseen classes read -3"""
    x = synth.make_images(B, H, W, seed=61)
    t = synth.make_labels(B, H, W, K, seed=62, block=8)
    t[:, -3:, :] = datasets.PAD_LABEL
    if hide:
        t[np.isin(t, UNSEEN)] = HIDDEN
    else:
        t[np.isin(t, UNSEEN)] = 0
    return cu(x), cu(t)


def fresh(kind="fcn32s", train=False, **kw):
    m = KINDS[kind](E)
    m.load_synthetic(1337, device=torch.device("cuda"))
    m.train() if train else m.eval()
    kw.setdefault("precision", torch.float32)
    return engine.TrainStep(m, EMB, optimizer="adam", lr=1e-5, **kw)


@pytest.mark.parametrize("kind,precision,loss", [("fcn32s", torch.float32, "cos"), ("fcn8s", torch.float32, "cos"),
                                                 ("fcn32s", torch.bfloat16, "mse")])
def test_step_trains_on_the_relabelled_target(kind, precision, loss):
    x, t = batch()
    assert (t == HIDDEN).any() and (t == -1).any() and (t == -2).any() and not torch.isin(t, cu(np.array(UNSEEN))).any()
    ts = fresh(kind, precision=precision, loss=loss, pseudo=CFG)
    ts.keep_ctx = True
    lossv, pred = ts.step(x, t)
    stride = 8 if kind == "fcn8s" else 32
    fmap = ts.last_fuse3 if kind == "fcn8s" else ts.last_ctx.coarse
    assert L.last_kernel() != "pseudo_relabel_kernel"                       # (the head, the backward pass and the optimizer came after)
    tp = ts.last_pseudo_target
    # heads.pseudo on the step's own map reproduces the step's target bit for bit
    want, ex = heads.pseudo(stride, fmap, ts.emb, H, W, t, UNSEEN, gamma=CFG["gamma"], keep=CFG["keep"], conf_floor=CFG["conf_floor"],
                            want=("counts", "cand", "thr"))
    assert L.last_kernel() == "pseudo_relabel_kernel" and L.prev_kernel() == "pseudo_thr_kernel"
    assert tp is not t and torch.equal(tp, want)
    changed = tp != t
    assert changed.any() and torch.equal(changed, (t == HIDDEN) & (tp >= 0)) and torch.isin(tp[changed], cu(np.array(UNSEEN))).all()
    assert torch.equal(ex["cand"] >= 0, t == HIDDEN)                          # gamma 2.5, no floor: every hidden pixel is a candidate
    assert torch.equal(ts.pseudo_counts, ex["counts"]) and int(ex["counts"][:, 1].sum()) == int(changed.sum())
    n, sel = ex["counts"][:, 0].cpu().numpy(), ex["counts"][:, 1].cpu().numpy()
    assert (n[UNSEEN] > 0).any() and n.sum() == n[UNSEEN].sum() and (sel >= (n * 300 + 999) // 1000).all() and (sel <= n).all()
    # loss, stats and prediction are the plain fused head's on (that map, that target)
    pred2 = torch.empty_like(pred)
    loss2, stats2 = torch.empty(1, device="cuda"), torch.empty(B, 2, device="cuda")
    heads.embed(loss, stride, fmap, ts.emb, H, W, pred2, tp, loss2, stats2)
    torch.cuda.synchronize()
    assert torch.equal(loss2.reshape(()), lossv) and torch.equal(stats2, ts.stats) and torch.equal(pred2, pred)
    assert stats2[:, 1].sum().item() == float((tp >= 0).sum()) > float((t >= 0).sum())
    # the train metrics keep the caller's target: the pseudo-labelled pixels are not counted
    assert torch.equal(ts.hist[0], utils.confusion_hist_device(t, pred, K)[0]) and int(ts.hist[0].sum()) == int((t >= 0).sum())
    # the counts accumulate until the caller zeroes them
    ts.step(x, t)
    assert int(ts.pseudo_counts[:, 0].sum()) == 2 * int(n.sum())
    ts.pseudo_counts.zero_()
    ts.set_pseudo_active(False)
    ts.step(x, t)
    assert not ts.pseudo_counts.any() and int(ts.stats[:, 1].sum()) == int((t >= 0).sum())


def test_referee_route_receives_the_relabelled_target():
    """fused_head=False: the materialised head reads the same relabelled target -- same map, same kernel, so the same labels and pixel
    counts; the two heads' losses are two fp32 evaluations of one mean of cosines (each within helpers_msinfer.bound, ~3e-5 at E = 20,
    of the exact value), compared at 1e-4"""
    x, t = batch()
    out = []
    for fused in (True, False):
        ts = fresh(fused_head=fused, pseudo=CFG)
        ts.keep_ctx = True
        lossv, pred = ts.step(x, t)
        out.append((float(lossv), ts.last_pseudo_target.clone(), ts.stats.clone()))
    assert (out[0][1] != t).any() and torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][2][:, 1], out[1][2][:, 1])
    assert out[0][2][:, 1].sum().item() == float((out[0][1] >= 0).sum())
    assert abs(out[0][0] - out[1][0]) <= 1e-4


def _state(ts, x, t, steps=2):
    for _ in range(steps):
        lossv, pred = ts.step(x, t)
    torch.cuda.synchronize()
    return float(lossv), pred.clone(), ts.flat_w.clone(), ts.flat_b.clone()


def _same(a, b):
    return a[0] == b[0] and all(torch.equal(u, v) for u, v in zip(a[1:], b[1:]))


def test_without_hidden_pixels_or_inactive_the_step_is_the_plain_step():
    """Dropout2d on (train mode): the mask generator is counter-based and seeded, so identically built steps draw the same masks"""
    x, t_plain = batch(hide=False)
    _, t_hidden = batch(hide=True)
    assert not (t_plain == HIDDEN).any()
    ref_plain = _state(fresh(train=True), x, t_plain)
    assert _same(_state(fresh(train=True, pseudo=CFG), x, t_plain), ref_plain)            # active, nothing hidden: nothing relabelled
    ref_hidden = _state(fresh(train=True), x, t_hidden)
    off = fresh(train=True, pseudo=CFG)
    off.set_pseudo_active(False)
    assert _same(_state(off, x, t_hidden), ref_hidden) and off.last_pseudo_target is None and not off.pseudo_counts.any()
    on = _state(fresh(train=True, pseudo=CFG), x, t_hidden)                               # and active with hidden pixels it is not
    assert on[0] != ref_hidden[0] and not torch.equal(on[2], ref_hidden[2])
    with pytest.raises(L.SznError):
        fresh().set_pseudo_active(True)
    fresh().set_pseudo_active(False)


def test_sim_ce_counts_the_pseudo_labelled_pixels_only_when_active():
    x, t = batch()
    ts = fresh(loss="sim_ce", sim_exclude=UNSEEN, pseudo=CFG)
    ts.keep_ctx = True
    n_seen = (t >= 0).sum(dim=(1, 2)).float()                                 # (the target holds no unseen label: they are hidden)
    assert ts._sim_kw["exclude"] == []
    ts.step(x, t)
    tp = ts.last_pseudo_target
    n_sel = ((tp != t).sum(dim=(1, 2))).float()
    assert n_sel.sum() > 0 and torch.equal(ts.stats[:, 1], n_seen + n_sel)
    ts.set_pseudo_active(False)
    assert ts._sim_kw["exclude"] == UNSEEN
    ts.step(x, t)
    assert torch.equal(ts.stats[:, 1], n_seen)
    ts.set_pseudo_active(True)
    ts.step(x, t)
    assert (ts.stats[:, 1] > n_seen).any()


def test_existing_heads_ignore_the_hidden_label_like_the_padding_label():
    x, t3 = batch()
    t2 = torch.where(t3 == HIDDEN, torch.full_like(t3, datasets.PAD_LABEL), t3)
    assert (t3 == HIDDEN).any() and not (t2 == HIDDEN).any()
    m = models.FCN32s(E).load_synthetic(1337, device=torch.device("cuda")).eval()
    for loss in ("cos", "mse", "sim_ce"):
        a = [v.clone() for v in m.embed_predict(x, EMB, t3, loss=loss)]
        b = m.embed_predict(x, EMB, t2, loss=loss)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.isfinite(a[0]), loss
    a = [v.clone() for v in m.seenmask_predict(x, t3, K, UNSEEN)]
    b = m.seenmask_predict(x, t2, K, UNSEEN)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    pred = m.embed_predict(x, EMB)[1].clone()
    assert torch.equal(utils.confusion_hist_device(t3, pred, K, UNSEEN), utils.confusion_hist_device(t2, pred, K, UNSEEN))
    mc = models.FCN32s(K).load_synthetic(1337, device=torch.device("cuda")).eval()
    a = [v.clone() for v in mc.softmax_predict(x, t3)]
    b = mc.softmax_predict(x, t2)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # the materialised losses too
    with torch.no_grad():
        score = m(x, mode='fcn')
        emb = cu(EMB)
        for fn in (utils.cosine_loss, utils.mse_loss):
            assert torch.equal(fn(score, t3, emb), fn(score, t2, emb))


def test_augmentation_carries_a_hidden_region_through():
    rng = np.random.RandomState(7)
    h, w = 40, 56
    img = rng.randint(0, 256, (2, h, w, 3)).astype(np.uint8)
    lbl = rng.randint(0, K, (2, h, w)).astype(np.int64)
    lbl[:, 10:30, 20:44] = HIDDEN
    lbl[:, :2, :] = -1
    # scale 1, no flip, crop = the image: the labels come back as they went in
    rec = np.array([datasets.Augment.record(h, w, 1.0, crop=(h, w))] * 2, dtype=np.int32)
    _, out = utils.augment_to_device(img, lbl, rec, (h, w))
    assert torch.equal(out.cpu(), torch.from_numpy(lbl))
    # scaled by 1.5, mirrored, cropped, and scaled by 0.5 with padding: nearest-index copies -- no new value appears, -3 survives
    rec = np.array([datasets.Augment.record(h, w, 1.5, 0.5, 0.5, True, crop=(48, 48)), datasets.Augment.record(h, w, 0.5, crop=(48, 48))],
                   dtype=np.int32)
    _, out = utils.augment_to_device(img, lbl, rec, (48, 48))
    out = out.cpu().numpy()
    for b in range(2):
        assert set(np.unique(out[b])) <= set(np.unique(lbl[b])) | {datasets.PAD_LABEL}
        assert (out[b] == HIDDEN).sum() > 20
    assert (out[1] == datasets.PAD_LABEL).any()


def _trainer(tmp, m=None, **kw):
    m = m if m is not None else models.FCN32s(E).load_synthetic(1337, device=torch.device("cuda"))
    ds = SyntheticSegmentation(split="train_seen", n_images=2, size=(H, W), n_class=K, embed_dim=E, unseen=UNSEEN, seed=5, hide_unseen=True)
    loader = torch.utils.data.DataLoader(ds, batch_size=2, shuffle=False)
    layers = models.opt_layers(m)
    opt = optim.FusedAdam([{"params": [getattr(m, n).weight for n in layers]},
                           {"params": [getattr(m, n).bias for n in layers], "lr": 2e-5}], lr=1e-5)
    args = dict(cuda=True, model=m, optimizer=opt, train_loader=loader, val_loader=loader, log_dir=str(tmp), dataset="pascal",
                max_epoch=2, tb_writer=None, pixel_embeddings=E, loss_func="cos", unseen=UNSEEN, val_unseen=UNSEEN[1:], embed_arr=EMB)
    args.update(kw)
    return ds, trainer_fcn.Trainer(**args)


def test_trainer_starts_self_training_at_its_epoch(fast_tmp):
    tmp = pathlib.Path(fast_tmp)
    ds, t = _trainer(tmp / "run", pseudo=dict(keep=0.3, gamma=2.5), pseudo_start_epoch=1)
    hidden = sum(int((ds[i][1][0] == HIDDEN).sum()) for i in range(len(ds)))
    assert hidden > 0
    for epoch in (0, 1):
        t.epoch = epoch
        t.train_epoch()
    lines = open(tmp / "run" / "pseudo_log.csv").read().strip().split("\n")
    assert lines[0] == "epoch,class,candidates,selected"
    rows = [[int(v) for v in ln.split(",")] for ln in lines[1:]]
    assert [r[:2] for r in rows] == [[e, k] for e in (0, 1) for k in UNSEEN]
    assert all(r[2] == 0 and r[3] == 0 for r in rows[:3])                                # epoch 0: not started
    assert sum(r[2] for r in rows[3:]) == hidden and sum(r[3] for r in rows[3:]) > 0      # epoch 1: every hidden pixel a candidate
    assert all(r[3] >= (r[2] * 300 + 999) // 1000 for r in rows[3:])
    assert t._step._pseudo["gamma"] == 2.5 and t._step._pseudo_active
    # gamma defaults to the trainer's calibration
    _, t2 = _trainer(tmp / "cal", t.model, pseudo=dict(keep=0.5), calibration=0.125, rank=1)
    assert t2.pseudo["gamma"] == 0.125 and t2.pseudo["unseen"] == UNSEEN
    _, t3 = _trainer(tmp / "nocal", t.model, pseudo=dict(keep=0.5), rank=1)
    assert t3.pseudo["gamma"] == 0.0
    # refused at construction
    for over in (dict(unseen=[], val_unseen=[]), dict(pixel_embeddings=None, loss_func="cross_entropy"), dict(pseudo=dict(keep=1.5)),
                 dict(pseudo=dict(keep=0.3, gamma=float("nan"))), dict(fused_step=False)):
        with pytest.raises(L.SznError):
            _trainer(tmp / "bad", t.model, **dict(dict(pseudo=dict(keep=0.3), rank=1), **over))


def test_cli_pseudo_label_in_a_child_process(fast_tmp):
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--synthetic", "2", "64", "64", "-c", "4", "-tu", "1,13", "-vu", "17,19", "--pseudo-label",
           "0.3", "--pseudo-gamma", "2.5", "-ve", "1", "-dir", fast_tmp, "-n", "pl", "--workers", "0", "--batch-size", "2"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    log = glob.glob(os.path.join(fast_tmp, "logs", "pl_CFG_4_*"))[0]
    lines = open(os.path.join(log, "pseudo_log.csv")).read().strip().split("\n")
    unseen = [1, 13, 17, 19]                                   # (configuration 4 has no seen-mask phase: one FCN epoch, one validation)
    rows = [[int(v) for v in ln.split(",")] for ln in lines[1:]]
    assert lines[0] == "epoch,class,candidates,selected" and [r[:2] for r in rows] == [[0, k] for k in unseen]
    assert all(r[3] <= r[2] for r in rows)
