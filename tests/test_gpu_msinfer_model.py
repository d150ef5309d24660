"""GPU: multi-scale / mirrored inference through the model surface (FCN32s / FCN8s .ms_predict), the trainer (eval_scales, eval_flip)
and the CLI (--eval-scales, --eval-flip), on a small synthetic input (33 x 47, B = 2).  The prediction is compared with the float64
restatement (tests/helpers_msinfer.py) built from the very maps the network produced for each view, outside the margin rule of
tests/test_gpu_msinfer.py: equal wherever the reference's top-2 margin exceeds twice the accumulation bound."""
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
import helpers_msinfer as HM  # noqa: E402
from zeroshotsemanticsegmentation_amd import _lib as L  # noqa: E402
from zeroshotsemanticsegmentation_amd import heads, models, optim, synth, trainer_fcn, utils  # noqa: E402
from zeroshotsemanticsegmentation_amd.synthetic_dataset import SyntheticSegmentation  # noqa: E402

E, K, B, H, W = 20, 33, 2, 33, 47
UNSEEN = [0, 12, 16, 18]
EMB = np.load(os.path.join(ROOT, "tests", "golden", "embeddings_context_20.npy"))


@functools.lru_cache(maxsize=None)
def net(kind="fcn32s"):
    cls = {"fcn32s": models.FCN32s, "fcn8s": models.FCN8s}[kind]
    return cls(E).load_synthetic(1337, device=torch.device("cuda")).eval()


@functools.lru_cache(maxsize=None)
def batch():
    x = torch.from_numpy(synth.make_images(B, H, W, seed=31)).cuda()
    t = synth.make_labels(B, H, W, K, seed=32, block=8)
    t[:, :2, :3] = -1
    return x, torch.from_numpy(t).cuda()


def reference(m, x, scales, flip, mode=0, gmap=None, target=None):
    """the float64 restatement on the maps the network gives for each view of x"""
    views, stride = [], None
    with torch.no_grad():
        for Hs, Ws, f in heads.ms_views(H, W, scales, flip):
            _, stride, fmap = m._head_map(heads.resize_flip(x, Hs, Ws, f))
            views.append((fmap.float().cpu().numpy()[..., :E].copy(), Hs, Ws, f))
    ref = HM.reference(stride, H, W, views, EMB, UNSEEN, mode, None if gmap is None else gmap.cpu().numpy(),
                       None if target is None else target.cpu().numpy())
    ref["clear"] = ref["margin"] > 2 * HM.bound(len(views), ref["kappa"], E)
    return ref


def check(pred, ref, what):
    p = pred.cpu().numpy()
    print("%s: %.2f %% of the pixels inside the margin, kappa max %.3f" % (what, 100 * (1 - ref["clear"].mean()), np.nanmax(ref["kappa"])))
    assert p.dtype == np.int64 and p.shape == (B, H, W)
    # the margin rule of tests/test_gpu_msinfer.py, share included: the maps come from the network, so kappa and with it the bound are
    # not the test's to choose, and a comparison that most pixels had dropped out of would show nothing
    assert 1 - ref["clear"].mean() <= 0.05
    assert np.array_equal(p[ref["clear"]], ref["pred"][ref["clear"]])


def test_identity_view_is_embed_predict():
    m = net()
    x, t = batch()
    loss0, _ = m.embed_predict(x, EMB, t)
    loss, pred = m.ms_predict(x, EMB, scales=(1.0,), flip=False, target=t)
    assert torch.equal(loss, loss0) and loss.dim() == 0
    check(pred, reference(m, x, (1.0,), False), "identity")
    l2, p2 = m.ms_predict(x, EMB, scales=(1.0,))
    assert l2 is None and torch.equal(p2, pred)
    lm, pm = m.ms_predict(x, EMB, scales=(1.0,), target=t, loss="mse")
    assert torch.equal(lm, m.embed_predict(x, EMB, t, loss="mse")[0]) and torch.equal(pm, pred)


def test_three_scales_and_mirror_match_the_reference():
    m = net()
    x, t = batch()
    loss, pred = m.ms_predict(x, EMB, scales=(1.5, 0.5, 1.0), flip=True, target=t)
    assert L.last_kernel() == "ms_pixel_kernel"                             # (before the next call launches something else)
    assert torch.equal(loss, m.embed_predict(x, EMB, t)[0])
    check(pred, reference(m, x, (0.5, 1.0, 1.5), True), "3 scales + mirror")


@pytest.mark.parametrize("group", ["seenmask", "target"])
def test_grouped_modes_match_the_reference(group):
    m = net()
    x, t = batch()
    loss, pred = m.ms_predict(x, EMB, scales=(0.5, 1.0), flip=True, target=t, unseen=UNSEEN, group=group)
    loss0, _ = m.szn_predict(x, EMB, UNSEEN, t, group=group)
    assert torch.equal(loss, loss0)
    if group == "seenmask":
        gmap = m._last_group
        assert gmap is not None and tuple(gmap.shape) == (B, H, W)
        check(pred, reference(m, x, (0.5, 1.0), True, 1, gmap=gmap), "seenmask group")
    else:
        check(pred, reference(m, x, (0.5, 1.0), True, 2, target=t), "target group")


def test_fcn8s_runs_the_stride_8_form():
    m = net("fcn8s")
    x, t = batch()
    loss, pred = m.ms_predict(x, EMB, scales=(0.5, 1.0), flip=True, target=t)
    assert torch.equal(loss, m.embed_predict(x, EMB, t)[0])
    ref = reference(m, x, (0.5, 1.0), True)
    assert m._head_map(x)[1] == 8
    check(pred, ref, "fcn8s")


def test_refused_configurations():
    m = net()
    x, t = batch()
    with pytest.raises(L.SznError) as ei:
        m.ms_predict(x, EMB, scales=(0.5, 1.5))
    assert "1.0" in str(ei.value)
    with pytest.raises(L.SznError) as ei:
        m.ms_predict(x, None, scales=(1.0,))
    assert "softmax" in str(ei.value)
    with pytest.raises(L.SznError):
        m.ms_predict(x, EMB, scales=(1.0,), loss="cross_entropy")
    with pytest.raises(L.SznError):
        m.ms_predict(x, EMB, scales=(1.0,), group="target", unseen=UNSEEN)          # forced unseen needs the target


def _trainer(tmp, **kw):
    m = models.FCN32s(E).load_synthetic(1337, device=torch.device("cuda"))
    ds = SyntheticSegmentation(split="val", n_images=4, size=(H, W), n_class=K, embed_dim=E, seed=5)
    loader = torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False)
    ws = [getattr(m, n).weight for n in models._OPT_LAYERS]
    bs = [getattr(m, n).bias for n in models._OPT_LAYERS]
    opt = optim.FusedAdam([{"params": ws}, {"params": bs, "lr": 2e-5}], lr=1e-5)
    t = trainer_fcn.Trainer(cuda=True, model=m, optimizer=opt, train_loader=loader, val_loader=loader, log_dir=str(tmp),
                            dataset="context", max_epoch=1, tb_writer=None, pixel_embeddings=E, loss_func="cos", unseen=UNSEEN,
                            val_unseen=[16, 18], **kw)
    return m, loader, t


def _row_vs(tmp, t, loader, predict):
    row = open(os.path.join(str(tmp), "val_log.csv")).read().strip().split("\n")[1].split(",")
    lts, lps, losses = [], [], []
    for data, target in loader:
        data, lbl, _ = t._unpack(data, target)
        loss, pred = predict(data, lbl)
        lts.append(lbl[0].cpu().numpy()); lps.append(pred[0].cpu().numpy()); losses.append(float(loss))
    want, seen_m, unseen_m = utils.label_accuracy_score(lts, lps, K, unseen=[16, 18])
    got = np.array([float(v) for v in row[2:15]])
    np.testing.assert_allclose(got, np.array([np.mean(losses)] + list(want) + list(seen_m) + list(unseen_m)), rtol=1e-6, equal_nan=True)
    return lps


def test_trainer_validates_over_the_views(fast_tmp):
    tmp_path = pathlib.Path(fast_tmp)            # validate() writes a full checkpoint per call
    m, loader, t = _trainer(tmp_path / "ms", eval_scales=(0.5, 1.0), eval_flip=True)
    assert t.eval_scales == (0.5, 1.0) and t.eval_flip is True
    t.validate()
    m.eval()
    ms = _row_vs(tmp_path / "ms", t, loader, lambda d, l: m.ms_predict(d, t.embeddings, (0.5, 1.0), True, l))
    # without the keywords: the single-view row, as before
    m1, loader1, t1 = _trainer(tmp_path / "one")
    assert t1.eval_scales is None and t1.eval_flip is False
    t1.validate()
    m1.eval()
    one = _row_vs(tmp_path / "one", t1, loader1, lambda d, l: m1.embed_predict(d, t1.embeddings, l))
    # the routes themselves: the ensemble head's kernel is the last launch of a prediction only with the keywords
    data, target = next(iter(loader))
    t._predict_device(data, target, False)
    assert L.last_kernel() == "ms_pixel_kernel"
    t1._predict_device(data, target, False)
    assert L.last_kernel() != "ms_pixel_kernel"
    assert len(ms) == len(one) == 4
    # a softmax configuration has no view ensemble
    with pytest.raises(L.SznError):
        trainer_fcn.Trainer(cuda=True, model=m1, optimizer=t1.optim, train_loader=loader1, val_loader=loader1,
                            log_dir=str(tmp_path / "ce"), dataset="context", max_epoch=1, tb_writer=None, pixel_embeddings=None,
                            loss_func="cross_entropy", eval_scales=(1.0,))


def test_cli_eval_scales_in_a_child_process(fast_tmp):
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--synthetic", "4", "33", "47", "-c", "18", "--eval-scales", "0.5", "1",
           "--eval-flip", "-ve", "1", "-dir", fast_tmp, "-n", "ms", "--workers", "0"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    log = glob.glob(os.path.join(fast_tmp, "logs", "ms_CFG_18_*"))[0]
    rows = open(os.path.join(log, "val_log.csv")).read().strip().split("\n")
    assert len(rows) == 2 and "overall mean_iu" in r.stdout
