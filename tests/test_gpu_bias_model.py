"""GPU: the unseen-bias term through engine.TrainStep(loss="sim_ce", bias=...), the trainer and train.py --bias-loss, on synthetic
96 x 96 images, B = 2, K = 21, E = 20, three classes hidden.

  1. the step against the autograd route (forward -> utils.sim_ce_bias_loss -> backward), FCN32s and FCN8s, with the comparison and bounds
     of tests/test_gpu_mse_head.py part 3;
  2. set_bias_active(False): the plain sim_ce step, launch for launch, the same loss bits and the same parameter bits after one step;
  3. with pseudo= the head trains on last_pseudo_target (the referee on that target, exclude set emptied, `unseen` as given); with ohem=
     the hidden pixels are neither counted nor dropped;
  4. 20 Adam steps on one batch: fp32 (the loss falls and the hidden pixels' mean P_U rises), bf16 (finite), fp16 (finite dynamic scale,
     applied steps);
  5. the CLI: cfg 18 in bf16 with -loss sim_ce --bias-loss 0.5 runs an epoch plus validation on the fused route; --bias-loss without
     -loss sim_ce is refused.
"""
import glob
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers_bias as Bh  # noqa: E402
from zeroshotsemanticsegmentation_amd import _lib as L  # noqa: E402
from zeroshotsemanticsegmentation_amd import datasets, engine, models, synth, train, utils  # noqa: E402

E, K, B, H, W, T, LAM = 20, 21, 2, 96, 96, 0.1, 0.5
UNSEEN = [2, 5, 8]
HIDDEN = datasets.HIDDEN_LABEL
EMB = synth.make_embeddings(K, E)
SIM = dict(loss="sim_ce", sim_exclude=UNSEEN, sim_temperature=T)
BIAS = dict(unseen=UNSEEN, weight=LAM)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def batch(seed=61):
    x = synth.make_images(B, H, W, seed=seed)
    t = synth.make_labels(B, H, W, K, seed=seed + 1, block=8)
    t[:, -3:, :] = datasets.PAD_LABEL
    t[np.isin(t, UNSEEN)] = HIDDEN
    assert all((t[b] == HIDDEN).any() and (t[b] >= 0).any() for b in range(B))
    return cu(x), cu(t)


def fresh(cls=models.FCN32s, precision=torch.float32, keep_ctx=False, **kw):
    """keep_ctx: the step keeps last_pseudo_target / last_ohem_target (its backward pass then also keeps the forward state alive and is
    no longer the one the autograd comparison's bounds were set for)"""
    m = cls(E).load_synthetic(1337, device=torch.device("cuda")).eval()
    kw.setdefault("optimizer", "adam")
    kw.setdefault("lr", 1e-5)
    ts = engine.TrainStep(m, EMB, precision=precision, **kw)
    ts.keep_ctx = keep_ctx
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
    return names, lossv.clone(), pred.clone()


def _grad_rel(ma, mb, names):
    out = {}
    for n in names:
        for kind in ("weight", "bias"):
            out["%s.%s" % (n, kind)] = rel(getattr(getattr(mb, n), kind).grad, getattr(getattr(ma, n), kind).grad)
    return out


# ----------------------------------------------------------------------------------------------- 1. TrainStep vs the autograd route
@pytest.mark.parametrize("arch", ["fcn32s", "fcn8s"])
def test_train_step_vs_autograd_route(arch, monkeypatch):
    """the bounds of tests/test_gpu_mse_head.py part 3: loss 1e-6 relative; every layer's gradient on the same forward state 1e-4
    (FCN32s) / 1e-5 (FCN8s) of its maximum; the prediction may flip exact near-ties only (< 2e-3 of the pixels)"""
    cls = models.FCN32s if arch == "fcn32s" else models.FCN8s
    x, t = batch()
    ma = cls(E).load_synthetic(1337, device=torch.device("cuda")).eval()
    score = ma(x, mode="fcn")
    loss = utils.sim_ce_bias_loss(score, t, cu(EMB), UNSEEN, T, UNSEEN, LAM, HIDDEN)
    loss.backward()
    plain = utils.sim_ce_loss(score.detach(), t, cu(EMB), UNSEEN, T)
    apred = utils.infer_lbl_device(score.detach(), cu(EMB))
    ts = fresh(cls, optimizer="sgd", lr=1e-6, momentum=0.99, weight_decay=0.0005, bias=BIAS, **SIM)
    names, lb, pb = _launches(monkeypatch, ts, x, t)
    errs = _grad_rel(ma, ts.model, models.opt_layers(ts.model))
    loss = loss.detach()
    eloss = abs(float(lb) - float(loss)) / abs(float(loss))
    print("%s: loss %.9g autograd %.9g rel err %.3e (plain sim_ce %.9g); worst gradient err / max %.3e (%s)"
          % (arch, float(lb), float(loss), eloss, float(plain), max(errs.values()), max(errs, key=errs.get)))
    assert "szn_fused_simce_bias_head_prepared" in names and not any(n.startswith("szn_fused_simce_head") for n in names)
    assert abs(float(plain) - float(loss)) > 1e-3 * abs(float(loss))            # the hidden pixels carry weight in this batch
    assert torch.equal(ts.stats[:, 1], ((t >= 0) | (t == HIDDEN)).sum(dim=(1, 2)).float())
    assert float((pb != apred).float().mean()) < 2e-3
    assert eloss < 1e-6
    bound = 1e-4 if arch == "fcn32s" else 1e-5
    for k, e in errs.items():
        assert e < bound, (k, e)


# ----------------------------------------------------------------------------------------------- 2. inactive: the plain sim_ce step
def test_inactive_bias_is_the_plain_sim_ce_step(monkeypatch):
    x, t = batch()
    plain_ts = fresh(**SIM)
    plain = _launches(monkeypatch, plain_ts, x, t)
    off = fresh(bias=BIAS, **SIM)
    off.set_bias_active(False)
    got = _launches(monkeypatch, off, x, t)
    assert got[0] == plain[0] and "szn_fused_simce_head_prepared" in got[0]
    assert torch.equal(got[1].view(torch.int32), plain[1].view(torch.int32)) and torch.equal(got[2], plain[2])
    for (n, p), (_, q) in zip(plain_ts.model.named_parameters(), off.model.named_parameters()):
        assert torch.equal(p.detach().view(torch.int32), q.detach().view(torch.int32)), n
    # active again: the bias head, another loss
    off.set_bias_active(True)
    on = _launches(monkeypatch, off, x, t)
    assert "szn_fused_simce_bias_head_prepared" in on[0] and float(on[1]) != float(got[1])
    with pytest.raises(L.SznError):
        plain_ts.set_bias_active(True)
    plain_ts.set_bias_active(False)


# ----------------------------------------------------------------------------------------------- 3. pseudo labels and mining
def test_with_pseudo_labels_the_head_trains_on_the_relabelled_target(monkeypatch):
    x, t = batch()
    ts = fresh(keep_ctx=True, bias=BIAS, pseudo=dict(unseen=UNSEEN, gamma=2.5, keep=0.3, conf_floor=-2.0), **SIM)
    assert ts._sim_kw["exclude"] == [] and ts._sim_kw["bias"]["unseen"] == UNSEEN       # the exclude set empties, U stays as given
    ma = models.FCN32s(E).load_synthetic(1337, device=torch.device("cuda")).eval()
    with torch.no_grad():
        score = ma(x, mode="fcn")
    names, lossv, _ = _launches(monkeypatch, ts, x, t)
    assert names.index("szn_pseudo_head") < names.index("szn_fused_simce_bias_head_prepared")
    tp = ts.last_pseudo_target
    relabelled = tp != t
    assert relabelled.any() and bool((t[relabelled] == HIDDEN).all()) and bool(torch.isin(tp[relabelled], cu(np.array(UNSEEN))).all())
    still = tp == HIDDEN
    assert still.any()                                                         # some hidden pixels remain: they get the bias term
    assert torch.equal(ts.stats[:, 1], ((tp >= 0) | still).sum(dim=(1, 2)).float())
    want = utils.sim_ce_bias_loss(score, tp, cu(EMB), [], T, UNSEEN, LAM, HIDDEN)
    other = utils.sim_ce_bias_loss(score, t, cu(EMB), [], T, UNSEEN, LAM, HIDDEN)
    print("pseudo + bias: loss %.9g referee on the relabelled target %.9g (on the caller's target %.9g); %d px relabelled, %d still hidden"
          % (float(lossv), float(want), float(other), int(relabelled.sum()), int(still.sum())))
    assert abs(float(lossv) - float(want)) < 1e-6 * abs(float(want))
    assert abs(float(other) - float(want)) > 1e-4 * abs(float(want))


def test_with_ohem_hidden_pixels_are_neither_counted_nor_dropped(monkeypatch):
    x, t = batch()
    ts = fresh(keep_ctx=True, bias=BIAS, ohem=dict(keep=0.25), **SIM)
    names, lossv, _ = _launches(monkeypatch, ts, x, t)
    assert bool(torch.isfinite(lossv)) and names.index("szn_ohem_head") < names.index("szn_fused_simce_bias_head_prepared")
    hid = t == HIDDEN
    tp = ts.last_ohem_target
    assert int(ts.ohem_counts[0]) == int((t >= 0).sum())                       # the labelled pixels alone (no class of UNSEEN is left in t)
    assert bool((tp[hid] == HIDDEN).all()) and (tp != t).any()
    assert torch.equal(ts.stats[:, 1], ((tp >= 0) | hid).sum(dim=(1, 2)).float())


# ----------------------------------------------------------------------------------------------- 4. it trains
def _mean_pu(m, x, t):
    with torch.no_grad():
        score = m(x, mode="fcn")
    pu = Bh.unseen_prob(score.double().cpu().numpy(), EMB, T, UNSEEN)[(t == HIDDEN).cpu().numpy()]
    only_hidden = torch.where(t == HIDDEN, t, torch.full_like(t, -1))
    nll = utils.sim_ce_bias_loss(score, only_hidden, cu(EMB), UNSEEN, T, UNSEEN, 1.0, HIDDEN)       # the referee: mean -log P_U
    return float(pu.mean()), float(nll)


@pytest.mark.parametrize("precision", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
def test_twenty_adam_steps(precision):
    x, t = batch(71)
    ts = fresh(precision=precision, bias=BIAS, **SIM)
    before = _mean_pu(ts.model, x, t) if precision == torch.float32 else None
    losses = [float(ts.step(x, t)[0]) for _ in range(20)]
    torch.cuda.synchronize()
    print("sim_ce + bias %s: loss %.6f -> %.6f" % (precision, losses[0], losses[-1]))
    assert all(np.isfinite(losses)), losses
    if precision == torch.float32:
        after = _mean_pu(ts.model, x, t)
        print("   hidden pixels: mean P_U %.6f -> %.6f, mean -log P_U %.6f -> %.6f" % (before[0], after[0], before[1], after[1]))
        assert losses[-1] < losses[0], losses
        assert after[0] > before[0] and after[1] < before[1], (before, after)
    if precision == torch.float16:
        assert ts.dynamic and np.isfinite(ts.loss_scale) and ts.loss_scale > 0 and ts.applied_steps > 0, (ts.loss_scale, ts.applied_steps)
        print("   fp16: scale %g (start 4096), applied steps %d of 20" % (ts.loss_scale, ts.applied_steps))


# ----------------------------------------------------------------------------------------------- 5. the CLI
def test_cli_bias_loss_epoch_and_validation(fast_tmp, monkeypatch):
    names, seen = [], []
    real = L.call

    def call(name, *a):                               # the weight and the hidden label the head is handed: arguments 20 and 21 behind the name
        names.append(name)
        if name.startswith("szn_fused_simce_bias_head"):
            seen.append((a[20], a[21]))
        return real(name, *a)
    monkeypatch.setattr(L, "call", call)
    train.main(['-c', '18', '-ve', '1', '-se', '1', '--batch-size', '2', '-n', 'bias', '--synthetic', '2', '64', '64', '--workers', '0',
                '-dir', fast_tmp, '-loss', 'sim_ce', '--bias-loss', '0.5', '--precision', 'bf16'])
    log = glob.glob(os.path.join(fast_tmp, 'logs', 'bias_CFG_18_*'))
    assert len(log) == 1 and 'FCN_LOSS_sim_ce' in log[0]
    rows = open(os.path.join(log[0], 'train_log.csv')).read().strip().split('\n')
    losses = [float(r.split(',')[2]) for r in rows[1:]]
    assert len(losses) >= 1 and all(np.isfinite(losses)), losses
    vrows = open(os.path.join(log[0], 'val_log.csv')).read().strip().split('\n')
    assert len(vrows) == 2 and np.isfinite(float(vrows[1].split(',')[2]))
    assert "szn_fused_simce_bias_head_prepared" in names                       # the step
    assert "szn_fused_simce_head" in names                                     # validation: no hidden pixels, the plain sim_ce head
    assert not any(n in ("szn_bilinear_up32_crop_fwd", "szn_bilinear_up_crop_fwd", "szn_cosine_loss_fwd", "szn_mse_loss_fwd") for n in names)
    assert seen and all(abs(wt - 0.5) < 1e-7 and hl == HIDDEN for wt, hl in seen), seen[:4]


def test_cli_refuses_the_bias_loss_without_sim_ce(fast_tmp):
    with pytest.raises(Exception) as ei:
        train.main(['-c', '18', '-ve', '1', '--synthetic', '2', '64', '64', '--workers', '0', '-dir', fast_tmp, '--bias-loss', '0.5'])
    assert "--bias-loss needs -loss sim_ce" in str(ei.value)
