"""GPU: the fused hinge ranking head (szn_fused_rank_head / _prepared) and train.py -loss rank on engine.TrainStep.

  1. the kernel against the materialised chain szn_bilinear_up_crop_fwd -> helpers_rank.rank_ref (float64) -> cast to f32 ->
     szn_bilinear_up_crop_bwd on the same coarse map: pred bit-equal to szn_fused_head_grouped's in group modes 0 / 1 / 2, counts exact,
     loss and stats within 1e-3 relative, |d(coarse) - chain| <= 1e-4 max|chain| + env elementwise, env = helpers_rank.rank_flip_envelope
     (the sub-gradient a float32 hinge within 1e-4 of its kink may take instead; asserted <= 5 % of max|chain|, identically zero at
     margin 2.5), for a uniform [-2, 2] map and a near-converged one (e_label + 1e-2 |e| noise), sum of hinges and hardest negative;
     16-bit d(coarse) within 1 ulp of the rounded f32 result, untouched padding channels, pred-only / loss-only calls,
     prepared == unprepared, two runs bit-identical;
  2. the head's own argument errors, with sentinel outputs that prove nothing was launched;
  3. TrainStep(loss="rank") against the autograd route (forward -> utils.rank_loss -> backward), FCN32s and FCN8s, both forms, with the
     comparison and bounds tests/test_gpu_mse_head.py part 3 uses;
  4. 20 Adam steps on one batch: fp32 (the loss falls), bf16 (finite), fp16 (finite dynamic scale, applied steps);
  5. the trainer and the CLI: cfg 18 in bf16 with --rank-margin 0.2 --rank-hardest and validation on the fused route, then -m test_all
     on the saved checkpoint; --rank-margin without -loss rank.

Measured on an MI355X: DESIGN.md section 7o.
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
import helpers_rank as R  # noqa: E402
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


def _args(fn, S, coarse, emb, H, W, c0, target, unseen, mode, gmap, exclude, margin, hardest, loss, stats, pred, dc, ws):
    B, h, w, ldc = coarse.shape
    K, E = emb.shape
    crop = models.CROP if S == 32 else models.CROP_UP8
    extra = (L.class_set(exclude), float(margin), int(hardest)) if "rank" in fn else ()
    return (fn, S, B, h, w, E, ldc, c0, H, W, crop, K, L.ptr(coarse), L.ptr(emb), L.ptr(target), L.class_set(unseen), mode,
            L.ptr(gmap)) + extra + (L.ptr(loss), L.ptr(stats), L.ptr(pred), L.dtype_code(dc.dtype) if dc is not None else 0, L.ptr(dc),
                                    L.ptr(ws), L.stream_ptr())


def _head(fn, S, coarse, emb, H, W, c0, target=None, unseen=None, mode=0, gmap=None, want_pred=True, dtype=None, ws=None,
          exclude=None, margin=0.1, hardest=0):
    """one call of szn_fused_rank_head / szn_fused_head_grouped (+ _prepared when `ws` holds the tables) -> loss, stats, pred, dcoarse"""
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
    L.call(*_args(fn, S, coarse, emb, H, W, c0, target, unseen, mode, gmap, exclude, margin, hardest, loss, stats, pred, dc, ws))
    return loss, stats, pred, dc


def _ordered16(t):
    """the bit patterns of a 16-bit float tensor as integers whose difference counts ulps (sign-magnitude -> two's complement)"""
    v = t.contiguous().view(torch.int16).to(torch.int32)
    mag = v & 0x7FFF
    return torch.where(v < 0, -mag, mag)


# ----------------------------------------------------------------------------------------------- 1. kernel vs materialised chain
@pytest.mark.parametrize("variant", R.VARIANTS, ids=lambda v: "%s_m%g_h%d" % v)
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "s%d_B%d_%dx%d_E%d_K%d" % c[:6])
def test_kernel_vs_materialised_chain(case, variant):
    """Measured on an MI355X (worst over CASES x VARIANTS): see DESIGN.md 7o."""
    S, B, H, W, E, K, c0, extra = case
    kind, margin, hardest = variant
    fn = "szn_fused_rank_head"
    I = R.inputs(case, kind, synth, G)
    crop, h, w, seed, exclude, tnp, emb_np = I["crop"], I["h"], I["w"], I["seed"], I["exclude"], I["target"], I["emb"]
    assert crop == (models.CROP if S == 32 else models.CROP_UP8)
    ldc = c0 + E + extra
    emb = cu(emb_np)
    t = cu(tnp)
    st = L.stream_ptr()
    unseen = [k for k in range(K) if k % 3 == 1]    # the grouping of modes 1 / 2: another set than `exclude`
    gmap = cu((np.random.RandomState(seed + 2).rand(B, H, W) < 0.5).astype(np.int64))
    coarse = torch.full((B, h, w, ldc), 123.0)
    coarse[..., c0:c0 + E] = torch.from_numpy(I["coarse"])
    coarse = coarse.cuda()
    # the materialised chain: upsample on the GPU, the loss and its gradient in float64 on the host, the transposed upsample on the GPU
    score = torch.empty(B, E, H, W, device="cuda")
    L.call("szn_bilinear_up_crop_fwd", S, B, h, w, E, ldc, c0, H, W, crop, L.ptr(coarse), L.ptr(score), st)
    torch.cuda.synchronize()
    score_np = score.cpu().numpy()
    oloss, ods, ostats = R.rank_ref(score_np, tnp, emb_np, exclude, margin, hardest)
    dscore = cu(ods.astype(np.float32))
    rdc = torch.zeros(B, h, w, ldc, device="cuda")
    L.call("szn_bilinear_up_crop_bwd", S, B, h, w, E, ldc, c0, H, W, crop, L.ptr(dscore), L.ptr(rdc), st)
    # the kink allowance: the reference's near-kink pairs, carried through the transposed upsample (non-negative weights) in float64
    env_s, pairs = R.rank_flip_envelope(score_np, tnp, emb_np, exclude, margin, hardest)
    Uy, Ux = R.up_matrices(S, h, w, H, W, crop)
    env = np.einsum("yi,xj,beyx->bije", Uy, Ux, env_s)
    # the fused head
    kw = dict(exclude=exclude, margin=margin, hardest=hardest)
    loss, stats, pred, dc = _head(fn, S, coarse, emb, H, W, c0, t, dtype=torch.float32, **kw)
    torch.cuda.synchronize()
    rdc_np = rdc[..., c0:c0 + E].double().cpu().numpy()
    dc_np = dc[..., c0:c0 + E].double().cpu().numpy()
    gmax = np.abs(rdc_np).max()
    diff = np.abs(dc_np - rdc_np)
    clear = diff[env == 0].max() if (env == 0).any() else 0.0
    print("%s %s: loss %.9g reference %.9g abs err %.3e; d(coarse): max |chain| %.3e, err / max %.3e (%.3e where env = 0), "
          "%d near-kink pairs, env / max %.3e" % (case, variant, float(loss), oloss, abs(float(loss) - oloss), gmax,
                                                  diff.max() / (gmax + 1e-300), clear / (gmax + 1e-300), pairs,
                                                  env.max() / (gmax + 1e-300)))
    counted = (tnp >= 0) & (tnp < K) & ~np.isin(tnp, exclude)
    assert np.array_equal(stats[:, 1].cpu().numpy(), ostats[:, 1]) and np.array_equal(ostats[:, 1], counted.sum(axis=(1, 2)))     # exact
    assert abs(float(loss) - oloss) <= 1e-3 * abs(oloss), (float(loss), oloss)
    assert np.abs(stats[:, 0].double().cpu().numpy() - ostats[:, 0]).max() <= 1e-3 * np.abs(ostats[:, 0]).max()
    assert env.max() <= 0.05 * gmax, (env.max(), gmax)          # the allowance cannot hide a failure
    if margin == 2.5:
        assert pairs == 0 and not env.any()
    assert (diff <= 1e-4 * gmax + env).all(), float((diff - env).max() / (gmax + 1e-300))
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
    p_only = _head(fn, S, coarse, emb, H, W, c0, **kw)[2]                      # pred-only: no target, no hinge
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


# ----------------------------------------------------------------------------------------------- 2. argument errors
@pytest.mark.parametrize("prepared", [False, True])
def test_argument_errors_launch_nothing(prepared):
    S, B, H, W, E, K = 32, 1, 40, 40, 20, 21
    crop = models.CROP
    h, w = (H + crop + S - 1) // S, (W + crop + S - 1) // S
    emb = cu(R.embeddings(K, E, synth, G))
    coarse = cu(synth.uniform(3, (B, h, w, E), -2, 2))
    t = cu(R.labels(B, H, W, K, [0], 4))
    fn = "szn_fused_rank_head" + ("_prepared" if prepared else "")
    lib = L.load()
    bad = [(None, -0.1, 0, "margin"), (None, float("nan"), 0, "margin"), (None, float("inf"), 1, "margin"),
           (None, 0.1, 2, "hardest"), (None, 0.1, -1, "hardest"),
           (list(range(K)), 0.1, 0, "competing"), (list(range(1, K)), 0.1, 1, "competing"), ([K], 0.1, 0, "exclude"),
           ([1, 255], 0.1, 0, "exclude")]
    for exclude, margin, hardest, word in bad:
        loss, stats = torch.full((1,), SENT, device="cuda"), torch.full((B, 2), SENT, device="cuda")
        pred = torch.full((B, H, W), -7, dtype=torch.int64, device="cuda")
        dc = torch.full((B, h, w, E), SENT, device="cuda")
        ws = torch.full((lib.szn_fused_head_workspace_bytes(B, h, w, E, K),), 0x5A, dtype=torch.uint8, device="cuda")
        a = _args(fn, S, coarse, emb, H, W, 0, t, None, 0, None, exclude, margin, hardest, loss, stats, pred, dc, ws)
        rc = getattr(lib, a[0])(*a[1:])
        assert rc == -1, (exclude, margin, hardest, rc)                      # SZN_ERR_ARG
        assert word in lib.szn_last_error().decode(), lib.szn_last_error()
        torch.cuda.synchronize()
        assert bool((loss == SENT).all()) and bool((stats == SENT).all()) and bool((pred == -7).all()) and bool((dc == SENT).all())
        assert bool((ws == 0x5A).all())                                      # not even the embedding tables were written


# ----------------------------------------------------------------------------------------------- 3. TrainStep vs the autograd route
E3, K3, H3, B3, M3 = 20, 21, 64, 2, 0.1
EXCL3 = [3, 9, 15]
KINK3 = 1e-5          # 25 x the float32 cosines' own error (below 4e-7 on every input measured)


def _grad_rel(ma, mb, names):
    out = {}
    for n in names:
        for kind in ("weight", "bias"):
            out["%s.%s" % (n, kind)] = rel(getattr(getattr(mb, n), kind).grad, getattr(getattr(ma, n), kind).grad)
    return out


def _step(m, emb, hardest, precision=torch.float32, **kw):
    return engine.TrainStep(m, emb, loss="rank", sim_exclude=EXCL3, rank_margin=M3, rank_hardest=hardest, precision=precision, **kw)


def _batch(seed):
    x = cu(synth.make_images(B3, H3, H3, seed=seed))
    t = cu(synth.make_labels(B3, H3, H3, K3, seed=seed + 1, block=16))
    return x, t


def _kink_allowance(cls, x, t, emb, score, hardest, names):
    """per parameter tensor: sum over the referee's near-kink pairs of |J' step|, J' = the backward pass of the network at this
    forward state (one pass per pair on a model of its own; the pass is linear in d(score))"""
    (b, y, x_), steps = R.rank_flip_pairs(score.detach().cpu().numpy(), t.cpu().numpy(), emb, EXCL3, M3, hardest, delta=KINK3)
    allow = {}
    if len(b):
        assert len(b) <= 16, len(b)                    # a handful of passes; more would mean the batch sits on its kinks
        mc = cls(E3).load_synthetic(1337, device=torch.device("cuda")).eval()
        for i in range(len(b)):
            mc.zero_grad()
            d = torch.zeros_like(score)
            d[b[i], :, y[i], x_[i]] = torch.from_numpy(steps[i]).to(d)
            mc(x, mode="fcn").backward(gradient=d)
            for n in names:
                for kind in ("weight", "bias"):
                    g = getattr(getattr(mc, n), kind).grad.detach().abs().double()
                    key = "%s.%s" % (n, kind)
                    allow[key] = g if key not in allow else allow[key] + g
    return len(b), allow


def _check_grads(ma, mb, names, bound, allow):
    """every layer: |g_b - g_a| <= bound max|g_a| + allowance elementwise, and the allowance itself <= 5 % of max|g_a|"""
    worst = 0.0
    for n in names:
        for kind in ("weight", "bias"):
            key = "%s.%s" % (n, kind)
            ga = getattr(getattr(ma, n), kind).grad.detach().double()
            gb = getattr(getattr(mb, n), kind).grad.detach().double()
            gmax = float(ga.abs().max())
            al = allow.get(key)
            if al is not None:
                assert float(al.max()) <= 0.05 * gmax, (key, float(al.max()), gmax)
            excess = (gb - ga).abs() - (al if al is not None else 0.0)
            worst = max(worst, float(excess.max()) / (gmax + 1e-300))
            assert float(excess.max()) <= bound * gmax, (key, float(excess.max()) / (gmax + 1e-300))
    return worst


@pytest.mark.parametrize("hardest", [False, True], ids=["sum", "hardest"])
@pytest.mark.parametrize("arch", ["fcn32s", "fcn8s"])
def test_train_step_vs_autograd_route(arch, hardest):
    """the comparison and bounds of tests/test_gpu_mse_head.py part 3, as the sim_ce step took them: loss 1e-6 relative; every layer's
    gradient on the same forward state within 1e-4 (FCN32s) / 1e-5 (FCN8s) of its maximum; the prediction may flip exact near-ties
    only (< 2e-3 of the pixels).
    The kinks: both routes evaluate the hinges in float32, so a hinge within the float32 cosine error of its kink may be active on one
    route and not on the other, and that moves every layer's gradient by the pixel's whole share -- J' (grad cos_k - grad cos_other) /
    (B N_b), far above 1e-5 of a layer's maximum on a batch of 2 x 64 x 64 pixels.  The allowance is derived from the referee alone:
    helpers_rank.rank_flip_pairs lists the hinges (and, for `hardest`, the top-two ties) of the autograd route's own score that lie
    within KINK3 = 1e-5 of a kink (25 x the measured float32 cosine error), each pair's step in d(score) goes through the network's
    backward pass on its own, and a layer may differ by bound x max + sum over pairs |J' step| elementwise.  So the bounds are the MSE
    step's wherever no kink is near, the allowance is asserted to stay below 5 % of each layer's maximum, and more than 16 pairs
    fail the test."""
    dev = torch.device("cuda")
    cls = models.FCN32s if arch == "fcn32s" else models.FCN8s
    emb = R.embeddings(K3, E3, synth, G)
    x, t = _batch(43)
    ma = cls(E3).load_synthetic(1337, device=dev).eval()
    mb = cls(E3).load_synthetic(1337, device=dev).eval()
    names = models.opt_layers(mb)
    score = ma(x, mode="fcn")
    loss = utils.rank_loss(score, t, cu(emb), EXCL3, M3, hardest)
    loss.backward()
    apred = utils.infer_lbl_device(score.detach(), cu(emb))
    pairs, allow = _kink_allowance(cls, x, t, emb, score, hardest, names)
    lb, pb = _step(mb, emb, hardest, optimizer="sgd", lr=1e-6, momentum=0.99, weight_decay=0.0005).step(x, t)
    torch.cuda.synchronize()
    errs = _grad_rel(ma, mb, names)
    eloss = abs(float(lb) - float(loss)) / abs(float(loss))
    print("%s hardest=%d: loss %.9g autograd %.9g rel err %.3e; worst gradient err / max %.3e (%s); %d hinges within %g of a kink"
          % (arch, hardest, float(lb), float(loss), eloss, max(errs.values()), max(errs, key=errs.get), pairs, KINK3))
    assert float(loss) > 0
    assert float((pb != apred).float().mean()) < 2e-3
    assert eloss < 1e-6
    bound = 1e-4 if arch == "fcn32s" else 1e-5
    worst = _check_grads(ma, mb, names, bound, allow)
    print("   worst gradient err beyond the kink allowance / max %.3e (bound %g)" % (worst, bound))
    if arch == "fcn8s":
        md = cls(E3).load_synthetic(1337, device=dev).eval().set_rank(EXCL3, M3, hardest)
        ld, pd = md.embed_loss(x, emb, t, loss="rank")                         # the autograd bridge with the fused stride-8 head
        ld.backward()
        torch.cuda.synchronize()
        assert torch.equal(pb, pd) and abs(float(ld) - float(loss)) < 1e-6 * abs(float(loss))
        _check_grads(ma, md, names, bound, allow)
    # inference: embed_predict(loss="rank") gives the step's kind of loss and the cosine route's prediction
    ma.set_rank(EXCL3, M3, hardest)
    with torch.no_grad():
        l2, p2 = ma.embed_predict(x, emb, t, loss="rank")
        _, p3 = ma.embed_predict(x, emb, t)
    assert torch.equal(p2, p3) and abs(float(l2) - float(loss)) < 1e-6 * abs(float(loss))


# ----------------------------------------------------------------------------------------------- 4. it trains
@pytest.mark.parametrize("precision", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
def test_twenty_adam_steps(precision):
    emb = R.embeddings(K3, E3, synth, G)
    x, t = _batch(71)
    m = models.FCN32s(E3).load_synthetic(1337, device=torch.device("cuda")).eval()
    ts = _step(m, emb, False, precision=precision, optimizer="adam", lr=1e-5)
    losses = [float(ts.step(x, t)[0]) for _ in range(20)]
    torch.cuda.synchronize()
    print("rank %s: loss %.6f -> %.6f" % (precision, losses[0], losses[-1]))
    assert all(np.isfinite(losses)), losses
    if precision == torch.float32:
        assert losses[-1] < losses[0], losses
    if precision == torch.float16:
        assert ts.dynamic and np.isfinite(ts.loss_scale) and ts.loss_scale > 0 and ts.applied_steps > 0, (ts.loss_scale, ts.applied_steps)
        print("   fp16: scale %g (start 4096), applied steps %d of 20" % (ts.loss_scale, ts.applied_steps))


# ----------------------------------------------------------------------------------------------- 5. trainer and CLI
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
        return any(n.startswith(("szn_fused_head_grouped", "szn_fused_head_strided", "szn_fused_head_prepared", "szn_fused_mse_head",
                                 "szn_fused_simce_head")) for n in self.names)


def test_cli_rank_epoch_and_test_all(fast_tmp, monkeypatch, capsys):
    rec = _Record(monkeypatch)
    seen = []
    real = L.call

    def call(name, *a):                               # the margin and the form the head is handed: arguments 18 and 19 behind the name
        if name.startswith("szn_fused_rank_head"):
            seen.append((a[18], a[19]))
        return real(name, *a)
    monkeypatch.setattr(L, "call", call)
    common = ['--synthetic', '2', '64', '64', '--workers', '0', '-dir', fast_tmp, '-loss', 'rank', '--rank-margin', '0.2', '--rank-hardest',
              '--precision', 'bf16']
    train.main(['-c', '18', '-ve', '1', '-se', '1', '--batch-size', '2', '-n', 'rk'] + common)
    log = glob.glob(os.path.join(fast_tmp, 'logs', 'rk_CFG_18_*'))
    assert len(log) == 1 and 'FCN_LOSS_rank' in log[0]
    rows = open(os.path.join(log[0], 'train_log.csv')).read().strip().split('\n')
    losses = [float(r.split(',')[2]) for r in rows[1:]]
    assert len(losses) >= 1 and all(np.isfinite(losses)), losses
    vrows = open(os.path.join(log[0], 'val_log.csv')).read().strip().split('\n')
    assert len(vrows) == 2 and np.isfinite(float(vrows[1].split(',')[2]))
    assert "szn_fused_rank_head_prepared" in rec.names and "szn_fused_rank_head" in rec.names        # the step, the validation
    assert not rec.materialised() and not rec.other_loss_head(), sorted(set(rec.names))
    assert seen and all(abs(m - 0.2) < 1e-7 and hd == 1 for m, hd in seen), seen[:4]
    run = os.path.basename(log[0])
    rec.names.clear()
    capsys.readouterr()
    train.main(['-c', '18', '-r', run, '-n', 'all', '-m', 'test_all'] + common)
    out = capsys.readouterr().out
    assert 'overall mean_iu' in out and 'unseen mean_iu' in out
    assert "szn_fused_rank_head" in rec.names and "szn_seenmask_head_k" in rec.names, sorted(set(rec.names))
    assert not rec.materialised() and not rec.other_loss_head(), sorted(set(rec.names))


def test_cli_refuses_the_margin_without_the_loss(fast_tmp):
    with pytest.raises(Exception) as ei:
        train.main(['-c', '18', '-ve', '1', '--synthetic', '2', '64', '64', '--workers', '0', '-dir', fast_tmp, '--rank-margin', '0.2'])
    assert "--rank-margin / --rank-hardest need -loss rank" in str(ei.value)
