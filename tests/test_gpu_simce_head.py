"""GPU: the fused similarity cross-entropy head (szn_fused_simce_head / _prepared) and train.py -loss sim_ce on engine.TrainStep.

  4. the kernel against the materialised chain szn_bilinear_up_crop_fwd -> helpers_simce.simce_ref (float64) -> cast to f32 ->
     szn_bilinear_up_crop_bwd on the same coarse map: pred bit-equal to szn_fused_head_grouped's in group modes 0 / 1 / 2, counts exact,
     loss within 1e-3 relative, d(coarse) within 1e-4 of the chain's maximum, for a uniform [-2, 2] map at T = 1 and T = 0.1 and a
     near-converged map (e_label + 1e-2 |e| noise, T = 0.1: the softmax saturates); 16-bit d(coarse) within 1 ulp of the rounded f32
     result, untouched padding channels, pred-only / loss-only calls, prepared == unprepared, two runs bit-identical;
  5. the head's own argument errors, with sentinel outputs that prove nothing was launched;
  6. TrainStep(loss="sim_ce") against the autograd route (forward -> utils.sim_ce_loss -> backward), FCN32s and FCN8s, with the
     comparison and bounds tests/test_gpu_mse_head.py part 3 uses;
  7. 20 Adam steps on one batch: fp32 (the loss falls), bf16 (finite), fp16 (finite dynamic scale, applied steps);
  8. the trainer and the CLI: cfg 18 in bf16 with validation on the fused route, then --calibration, --eval-flip and -m test_all on
     the saved checkpoint; --sim-temperature without -loss sim_ce.

Measured on an MI355X: DESIGN.md section 7k.
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
import helpers_simce as R  # noqa: E402
from zeroshotsemanticsegmentation_amd import _lib as L  # noqa: E402
from zeroshotsemanticsegmentation_amd import engine, models, synth, train, utils  # noqa: E402

G = os.path.join(ROOT, "tests", "golden")
SENT = -7.25          # sentinel of the channels outside [c0, c0 + E), and of outputs no launch may touch


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rel(a, b):
    a = a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)
    b = b.detach().double().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def same_bits(a, b):
    if a.is_floating_point():
        return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))
    return torch.equal(a, b)


def _emb(K, E):
    path = os.path.join(G, "embeddings_context_%d.npy" % E)
    if os.path.exists(path):
        e = np.load(path).astype(np.float32)
        if e.shape[0] >= K:
            return np.ascontiguousarray(e[:K])
    return synth.make_embeddings(K, E, seed=5)


def _args(fn, S, coarse, emb, H, W, c0, target, unseen, mode, gmap, exclude, T, loss, stats, pred, dc, ws):
    B, h, w, ldc = coarse.shape
    K, E = emb.shape
    crop = models.CROP if S == 32 else models.CROP_UP8
    extra = (L.class_set(exclude), float(T)) if "simce" in fn else ()
    return (fn, S, B, h, w, E, ldc, c0, H, W, crop, K, L.ptr(coarse), L.ptr(emb), L.ptr(target), L.class_set(unseen), mode,
            L.ptr(gmap)) + extra + (L.ptr(loss), L.ptr(stats), L.ptr(pred), L.dtype_code(dc.dtype) if dc is not None else 0, L.ptr(dc),
                                    L.ptr(ws), L.stream_ptr())


def _head(fn, S, coarse, emb, H, W, c0, target=None, unseen=None, mode=0, gmap=None, want_pred=True, dtype=None, ws=None,
          exclude=None, T=1.0):
    """one call of szn_fused_simce_head / szn_fused_head_grouped (+ _prepared when `ws` holds the tables) -> loss, stats, pred, dcoarse"""
    B, h, w, ldc = coarse.shape
    K, E = emb.shape
    dev = coarse.device
    loss = stats = dc = None
    if target is not None:
        loss, stats = torch.full((1,), -7.0, device=dev), torch.full((B, 2), -7.0, device=dev)
        if dtype is not None:
            dc = torch.full((B, h, w, ldc), SENT, device=dev, dtype=dtype)
    pred = torch.full((B, H, W), -7, dtype=torch.int64, device=dev) if want_pred else None
    if ws is None:
        ws = torch.empty(L.load().szn_fused_head_workspace_bytes(B, h, w, E, K), dtype=torch.uint8, device=dev)
    else:
        fn += "_prepared"
    L.call(*_args(fn, S, coarse, emb, H, W, c0, target, unseen, mode, gmap, exclude, T, loss, stats, pred, dc, ws))
    return loss, stats, pred, dc


def _ordered16(t):
    """the bit patterns of a 16-bit float tensor as integers whose difference counts ulps (sign-magnitude -> two's complement)"""
    v = t.contiguous().view(torch.int16).to(torch.int32)
    mag = v & 0x7FFF
    return torch.where(v < 0, -mag, mag)


# ----------------------------------------------------------------------------------------------- 4. kernel vs materialised chain
CASES = [  # stride, B, H, W, E, K, c0, padding channels behind
    (32, 2, 70, 101, 20, 33, 0, 42),          # border cells with missing taps
    (32, 1, 1, 1, 20, 21, 0, 44),             # a one-pixel image
    (32, 2, 97, 131, 300, 59, 3, 1),          # a channel offset, E not a multiple of 64
    (8, 3, 33, 47, 20, 150, 0, 12),           # stride 8, KP > 64: three 64-class rounds of the dense-A tile, the last one partial
    (8, 2, 64, 64, 20, 256, 0, 0),            # KP = 256
]
VARIANTS = [("uniform", 1.0), ("uniform", 0.1), ("converged", 0.1)]


def _coarse_map(kind, S, B, h, w, E, H, W, crop, emb, target, seed):
    if kind == "uniform":
        return synth.uniform(seed, (B, h, w, E), -2, 2)
    yy = np.clip(S * np.arange(h) + S // 2 - crop, 0, H - 1)
    xx = np.clip(S * np.arange(w) + S // 2 - crop, 0, W - 1)
    lab = target[:, yy][:, :, xx]
    lab = np.where((lab < 0) | (lab >= emb.shape[0]), 0, lab)
    base = emb[lab]
    nrm = np.linalg.norm(base, axis=-1, keepdims=True)
    noise = np.random.RandomState(seed + 7).randn(B, h, w, E).astype(np.float32)
    return (base + np.float32(1e-2) * nrm * noise).astype(np.float32)


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: "%s_T%g" % v)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "s%d_B%d_%dx%d_E%d_K%d" % c[:6])
def test_kernel_vs_materialised_chain(case, variant):
    """Measured on an MI355X (worst over CASES x VARIANTS): see DESIGN.md 7k."""
    S, B, H, W, E, K, c0, extra = case
    kind, T = variant
    fn = "szn_fused_simce_head"
    crop = models.CROP if S == 32 else models.CROP_UP8
    h, w = (H + crop + S - 1) // S, (W + crop + S - 1) // S
    ldc = c0 + E + extra
    seed = S * 1000 + E + K
    emb_np = _emb(K, E)
    emb = cu(emb_np)
    exclude = list(range(0, K, 3))                  # every third class does not compete
    tnp = R.labels(B, H, W, K, exclude, seed + 1)
    t = cu(tnp)
    st = L.stream_ptr()
    unseen = [k for k in range(K) if k % 3 == 1]    # the grouping of modes 1 / 2: another set than `exclude`
    gmap = cu((np.random.RandomState(seed + 2).rand(B, H, W) < 0.5).astype(np.int64))
    coarse = torch.full((B, h, w, ldc), 123.0)
    coarse[..., c0:c0 + E] = torch.from_numpy(_coarse_map(kind, S, B, h, w, E, H, W, crop, emb_np, tnp, seed))
    coarse = coarse.cuda()
    # the materialised chain: upsample on the GPU, the loss and its gradient in float64 on the host, the transposed upsample on the GPU
    score = torch.empty(B, E, H, W, device="cuda")
    L.call("szn_bilinear_up_crop_fwd", S, B, h, w, E, ldc, c0, H, W, crop, L.ptr(coarse), L.ptr(score), st)
    torch.cuda.synchronize()
    oloss, ods, ostats = R.simce_ref(score.cpu().numpy(), tnp, emb_np, exclude, T)
    dscore = cu(ods.astype(np.float32))
    rdc = torch.zeros(B, h, w, ldc, device="cuda")
    L.call("szn_bilinear_up_crop_bwd", S, B, h, w, E, ldc, c0, H, W, crop, L.ptr(dscore), L.ptr(rdc), st)
    # the fused head
    kw = dict(exclude=exclude, T=T)
    loss, stats, pred, dc = _head(fn, S, coarse, emb, H, W, c0, t, dtype=torch.float32, **kw)
    torch.cuda.synchronize()
    eloss = abs(float(loss) - oloss) / abs(oloss)
    egrad = rel(dc[..., c0:c0 + E], rdc[..., c0:c0 + E])
    print("%s %s: loss %.9g reference %.9g rel err %.3e; d(coarse) err / max %.3e" % (case, variant, float(loss), oloss, eloss, egrad))
    counted = (tnp >= 0) & (tnp < K) & ~np.isin(tnp, exclude)
    assert np.array_equal(stats[:, 1].cpu().numpy(), ostats[:, 1]) and np.array_equal(ostats[:, 1], counted.sum(axis=(1, 2)))     # exact
    assert eloss < 1e-3, (float(loss), oloss)
    assert rel(stats[:, 0], ostats[:, 0]) < 1e-3
    assert egrad < 1e-4
    assert bool((dc[..., :c0] == SENT).all()) and bool((dc[..., c0 + E:] == SENT).all())
    # pred: the cosine fused head's, bit for bit, in the three group modes; the loss does not depend on the group
    for mode in (0, 1, 2):
        gk = dict(target=t, unseen=unseen if mode else None, mode=mode, gmap=gmap if mode == 1 else None)
        ps = _head(fn, S, coarse, emb, H, W, c0, **gk, **kw)
        pc = _head("szn_fused_head_grouped", S, coarse, emb, H, W, c0, **gk)
        assert torch.equal(ps[2], pc[2]), mode
        assert same_bits(ps[0], loss) and same_bits(ps[1], stats), mode
        if mode == 0:
            assert torch.equal(ps[2], pred)
    p_only = _head(fn, S, coarse, emb, H, W, c0, **kw)[2]                      # pred-only: no target, no softmax
    assert torch.equal(p_only, pred)
    # 16-bit d(coarse): the fp32 result rounded to the type, to within 1 ulp (the store may round the scaled sum once); padding untouched
    for dt in (torch.bfloat16, torch.float16):
        _, _, p16, d16 = _head(fn, S, coarse, emb, H, W, c0, t, want_pred=False, dtype=dt, **kw)        # loss-only + dcoarse
        assert p16 is None
        want = dc[..., c0:c0 + E].to(dt)
        ulps = (_ordered16(d16[..., c0:c0 + E]) - _ordered16(want)).abs().max()
        assert int(ulps) <= 1, (dt, int(ulps))
        assert bool((d16[..., :c0] == SENT).all()) and bool((d16[..., c0 + E:] == SENT).all())
    # loss-only (no pred, no dcoarse), prepared == unprepared, and a second full call: the same bits
    l2, s2, _, _ = _head(fn, S, coarse, emb, H, W, c0, t, want_pred=False, **kw)
    ws = torch.empty(L.load().szn_fused_head_workspace_bytes(B, h, w, E, K), dtype=torch.uint8, device="cuda")
    L.call("szn_fused_head_prepare", E, K, L.ptr(emb), L.ptr(ws), st)
    outs = [_head(fn, S, coarse, emb, H, W, c0, t, dtype=torch.float32, ws=ws, **kw) for _ in range(2)]
    outs.append(_head(fn, S, coarse, emb, H, W, c0, t, dtype=torch.float32, **kw))
    torch.cuda.synchronize()
    assert same_bits(l2, loss) and same_bits(s2, stats)
    for o in outs:
        assert same_bits(o[0], loss) and same_bits(o[1], stats) and torch.equal(o[2], pred) and same_bits(o[3], dc)


# ----------------------------------------------------------------------------------------------- 5. argument errors
@pytest.mark.parametrize("prepared", [False, True])
def test_argument_errors_launch_nothing(prepared):
    S, B, H, W, E, K = 32, 1, 40, 40, 20, 21
    crop = models.CROP
    h, w = (H + crop + S - 1) // S, (W + crop + S - 1) // S
    emb = cu(_emb(K, E))
    coarse = cu(synth.uniform(3, (B, h, w, E), -2, 2))
    t = cu(R.labels(B, H, W, K, [0], 4))
    fn = "szn_fused_simce_head" + ("_prepared" if prepared else "")
    lib = L.load()
    bad = [(None, 0.0, "temperature"), (None, -1.0, "temperature"), (None, float("nan"), "temperature"),
           (list(range(K)), 0.1, "competing"), ([K], 0.1, "exclude"), ([1, 255], 0.1, "exclude")]
    for exclude, T, word in bad:
        loss, stats = torch.full((1,), SENT, device="cuda"), torch.full((B, 2), SENT, device="cuda")
        pred = torch.full((B, H, W), -7, dtype=torch.int64, device="cuda")
        dc = torch.full((B, h, w, E), SENT, device="cuda")
        ws = torch.full((lib.szn_fused_head_workspace_bytes(B, h, w, E, K),), 0x5A, dtype=torch.uint8, device="cuda")
        a = _args(fn, S, coarse, emb, H, W, 0, t, None, 0, None, exclude, T, loss, stats, pred, dc, ws)
        rc = getattr(lib, a[0])(*a[1:])
        assert rc == -1, (exclude, T, rc)                                    # SZN_ERR_ARG
        assert word in lib.szn_last_error().decode(), lib.szn_last_error()
        torch.cuda.synchronize()
        assert bool((loss == SENT).all()) and bool((stats == SENT).all()) and bool((pred == -7).all()) and bool((dc == SENT).all())
        assert bool((ws == 0x5A).all())                                      # not even the embedding tables were written


# ----------------------------------------------------------------------------------------------- 6. TrainStep vs the autograd route
E6, K6, H6, B6, T6 = 20, 21, 64, 2, 0.1
EXCL6 = [3, 9, 15]


def _grad_rel(ma, mb, names):
    out = {}
    for n in names:
        for kind in ("weight", "bias"):
            out["%s.%s" % (n, kind)] = rel(getattr(getattr(mb, n), kind).grad, getattr(getattr(ma, n), kind).grad)
    return out


def _step(m, emb, precision=torch.float32, **kw):
    return engine.TrainStep(m, emb, loss="sim_ce", sim_exclude=EXCL6, sim_temperature=T6, precision=precision, **kw)


def _batch(seed):
    x = cu(synth.make_images(B6, H6, H6, seed=seed))
    t = cu(synth.make_labels(B6, H6, H6, K6, seed=seed + 1, block=16))
    return x, t


@pytest.mark.parametrize("arch", ["fcn32s", "fcn8s"])
def test_train_step_vs_autograd_route(arch):
    """the bounds of tests/test_gpu_mse_head.py part 3: loss 1e-6 relative; every layer's gradient on the same forward state 1e-4
    (FCN32s) / 1e-5 (FCN8s) of its maximum; the prediction may flip exact near-ties only (< 2e-3 of the pixels)"""
    dev = torch.device("cuda")
    cls = models.FCN32s if arch == "fcn32s" else models.FCN8s
    emb = _emb(K6, E6)
    x, t = _batch(43)
    ma = cls(E6).load_synthetic(1337, device=dev).eval()
    mb = cls(E6).load_synthetic(1337, device=dev).eval()
    score = ma(x, mode="fcn")
    loss = utils.sim_ce_loss(score, t, cu(emb), EXCL6, T6)
    loss.backward()
    apred = utils.infer_lbl_device(score.detach(), cu(emb))
    lb, pb = _step(mb, emb, optimizer="sgd", lr=1e-6, momentum=0.99, weight_decay=0.0005).step(x, t)
    torch.cuda.synchronize()
    errs = _grad_rel(ma, mb, models.opt_layers(mb))
    eloss = abs(float(lb) - float(loss)) / abs(float(loss))
    print("%s: loss %.9g autograd %.9g rel err %.3e; worst gradient err / max %.3e (%s)"
          % (arch, float(lb), float(loss), eloss, max(errs.values()), max(errs, key=errs.get)))
    assert float((pb != apred).float().mean()) < 2e-3
    assert eloss < 1e-6
    bound = 1e-4 if arch == "fcn32s" else 1e-5
    for k, e in errs.items():
        assert e < bound, (k, e)
    if arch == "fcn8s":
        md = cls(E6).load_synthetic(1337, device=dev).eval().set_sim_ce(EXCL6, T6)
        ld, pd = md.embed_loss(x, emb, t, loss="sim_ce")                       # the autograd bridge with the fused stride-8 head
        ld.backward()
        torch.cuda.synchronize()
        assert torch.equal(pb, pd) and abs(float(ld) - float(loss)) < 1e-6 * abs(float(loss))
        for k, e in _grad_rel(ma, md, models.opt_layers(mb)).items():
            assert e < bound, (k, e)
    # inference: embed_predict(loss="sim_ce") gives the step's kind of loss and the cosine route's prediction
    ma.set_sim_ce(EXCL6, T6)
    with torch.no_grad():
        l2, p2 = ma.embed_predict(x, emb, t, loss="sim_ce")
        _, p3 = ma.embed_predict(x, emb, t)
    assert torch.equal(p2, p3) and abs(float(l2) - float(loss)) < 1e-6 * abs(float(loss))


# ----------------------------------------------------------------------------------------------- 7. it trains
@pytest.mark.parametrize("precision", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
def test_twenty_adam_steps(precision):
    emb = _emb(K6, E6)
    x, t = _batch(71)
    m = models.FCN32s(E6).load_synthetic(1337, device=torch.device("cuda")).eval()
    ts = _step(m, emb, precision=precision, optimizer="adam", lr=1e-5)
    losses = [float(ts.step(x, t)[0]) for _ in range(20)]
    torch.cuda.synchronize()
    print("sim_ce %s: loss %.6f -> %.6f" % (precision, losses[0], losses[-1]))
    assert all(np.isfinite(losses)), losses
    if precision == torch.float32:
        assert losses[-1] < losses[0], losses
    if precision == torch.float16:
        assert ts.dynamic and np.isfinite(ts.loss_scale) and ts.loss_scale > 0 and ts.applied_steps > 0, (ts.loss_scale, ts.applied_steps)
        print("   fp16: scale %g (start 4096), applied steps %d of 20" % (ts.loss_scale, ts.applied_steps))


# ----------------------------------------------------------------------------------------------- 8. trainer and CLI
class _Record(object):
    def __init__(self, monkeypatch):
        self.names = []
        real = L.call

        def call(name, *a):
            self.names.append(name)
            return real(name, *a)
        monkeypatch.setattr(L, "call", call)

    def materialised(self):
        return any(n in ("szn_bilinear_up32_crop_fwd", "szn_bilinear_up_crop_fwd", "szn_embed_argmax_k", "szn_cosine_loss_fwd",
                         "szn_mse_loss_fwd") for n in self.names)

    def other_loss_head(self):
        return any(n.startswith(("szn_fused_head_grouped", "szn_fused_head_strided", "szn_fused_head_prepared", "szn_fused_mse_head"))
                   for n in self.names)


def test_cli_sim_ce_epoch_and_validation_modes(fast_tmp, monkeypatch, capsys):
    rec = _Record(monkeypatch)
    common = ['--synthetic', '4', '64', '64', '--workers', '0', '-dir', fast_tmp, '-loss', 'sim_ce', '--sim-temperature', '0.1',
              '--precision', 'bf16']
    train.main(['-c', '18', '-ve', '1', '--batch-size', '2', '-n', 'sce'] + common)
    log = glob.glob(os.path.join(fast_tmp, 'logs', 'sce_CFG_18_*'))
    assert len(log) == 1 and 'FCN_LOSS_sim_ce' in log[0]
    rows = open(os.path.join(log[0], 'train_log.csv')).read().strip().split('\n')
    losses = [float(r.split(',')[2]) for r in rows[1:]]
    assert len(losses) >= 1 and all(np.isfinite(losses)), losses
    vrows = open(os.path.join(log[0], 'val_log.csv')).read().strip().split('\n')
    assert len(vrows) == 2 and np.isfinite(float(vrows[1].split(',')[2]))
    assert "szn_fused_simce_head_prepared" in rec.names and "szn_fused_simce_head" in rec.names        # the step, the validation
    assert not rec.materialised() and not rec.other_loss_head(), sorted(set(rec.names))
    run = os.path.basename(log[0])
    for name, extra, head in (("cal", ['-m', 'test_fcn', '--calibration', '0.1'], "szn_calib_head"),
                              ("flip", ['-m', 'test_fcn', '--eval-flip'], "szn_ms_head"),
                              ("all", ['-m', 'test_all'], "szn_seenmask_head_k")):
        rec.names.clear()
        capsys.readouterr()
        train.main(['-c', '18', '-r', run, '-n', name] + extra + common)
        out = capsys.readouterr().out
        assert 'overall mean_iu' in out and 'unseen mean_iu' in out, name
        assert "szn_fused_simce_head" in rec.names and head in rec.names, (name, sorted(set(rec.names)))
        assert not rec.materialised() and not rec.other_loss_head(), (name, sorted(set(rec.names)))


def test_cli_refuses_the_temperature_without_the_loss(fast_tmp):
    with pytest.raises(Exception) as ei:
        train.main(['-c', '18', '-ve', '1', '--synthetic', '4', '64', '64', '--workers', '0', '-dir', fast_tmp, '--sim-temperature', '0.1'])
    assert "--sim-temperature needs -loss sim_ce" in str(ei.value)
