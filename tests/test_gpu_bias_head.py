"""GPU: the fused sim_ce head with the unseen-bias term (szn_fused_simce_bias_head / _prepared).

  1. the kernel against the materialised chain szn_bilinear_up_crop_fwd -> helpers_bias.bias_ref (float64) -> cast to f32 ->
     szn_bilinear_up_crop_bwd on the same coarse map, on helpers_rank.CASES with about 20 % of the pixels hidden: pred bit-equal to
     szn_fused_head_grouped's in group modes 0 / 1 / 2, N_b exact, loss and stats within 1e-3 relative and d(coarse) within 1e-4 of its
     maximum -- the bounds of tests/test_gpu_simce_head.py part 4: the arithmetic is the same (expf, logf, the hardware reciprocal of n_k)
     -- for a uniform [-2, 2] map at T = 1 and 0.1 and a near-converged map whose positions all sit at seen classes (P_U small at the
     hidden pixels), weights 0.5 and 2; T = 0.01 on the one-pixel case, that pixel hidden and at a seen class's embedding (P_U below
     1e-30: no float32 number); 16-bit d(coarse) within 1 ulp of the rounded f32 result, untouched padding channels, pred-only /
     loss-only calls, prepared == unprepared, two runs bit-identical;
  2. a target without hidden pixels: every output is szn_fused_simce_head's bit for bit (loss, stats, pred, d(coarse) f32 and 16-bit);
  3. the head's own argument errors, with sentinel outputs that prove nothing was launched.

Measured on an MI355X: DESIGN.md section 7p.
"""
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
import helpers_rank as R  # noqa: E402
from zeroshotsemanticsegmentation_amd import _lib as L  # noqa: E402
from zeroshotsemanticsegmentation_amd import datasets, models, synth  # noqa: E402

G = os.path.join(ROOT, "tests", "golden")
SENT = -7.25          # sentinel of the channels outside [c0, c0 + E), and of outputs no launch may touch
HIDDEN = datasets.HIDDEN_LABEL
FN = "szn_fused_simce_bias_head"
# (map, T, weight); the last one runs on the one-pixel case only
VARIANTS = [("uniform", 1.0, 0.5), ("uniform", 0.1, 2.0), ("converged", 0.1, 0.5), ("converged", 0.01, 2.0)]
ONE_PIXEL = R.CASES[1]
PAIRS = [(c, v) for c in R.CASES for v in VARIANTS[:3]] + [(ONE_PIXEL, VARIANTS[3])]


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rel(a, b):
    a = a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)
    b = b.detach().double().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def same_bits(a, b):
    if a.is_floating_point():
        it = torch.int32 if a.dtype == torch.float32 else torch.int16
        return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(it), b.view(it))
    return torch.equal(a, b)


def _args(fn, S, coarse, emb, H, W, c0, target, unseen, mode, gmap, exclude, T, bias, loss, stats, pred, dc, ws):
    """bias = (unseen set, weight, hidden label) for the bias head, ignored by the others"""
    B, h, w, ldc = coarse.shape
    K, E = emb.shape
    crop = models.CROP if S == 32 else models.CROP_UP8
    extra = ()
    if "simce" in fn:
        extra = (L.class_set(exclude), float(T))
    if "bias" in fn:
        extra += (L.class_set(bias[0]), float(bias[1]), int(bias[2]))
    return (fn, S, B, h, w, E, ldc, c0, H, W, crop, K, L.ptr(coarse), L.ptr(emb), L.ptr(target), L.class_set(unseen), mode,
            L.ptr(gmap)) + extra + (L.ptr(loss), L.ptr(stats), L.ptr(pred), L.dtype_code(dc.dtype) if dc is not None else 0, L.ptr(dc),
                                    L.ptr(ws), L.stream_ptr())


def _head(fn, S, coarse, emb, H, W, c0, target=None, unseen=None, mode=0, gmap=None, want_pred=True, dtype=None, ws=None,
          exclude=None, T=0.1, bias=None):
    """one call of szn_fused_simce_bias_head / szn_fused_simce_head / szn_fused_head_grouped (+ _prepared when `ws` holds the tables)
    -> loss, stats, pred, dcoarse"""
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
    L.call(*_args(fn, S, coarse, emb, H, W, c0, target, unseen, mode, gmap, exclude, T, bias, loss, stats, pred, dc, ws))
    return loss, stats, pred, dc


def _ordered16(t):
    """the bit patterns of a 16-bit float tensor as integers whose difference counts ulps (sign-magnitude -> two's complement)"""
    v = t.contiguous().view(torch.int16).to(torch.int32)
    mag = v & 0x7FFF
    return torch.where(v < 0, -mag, mag)


def _padded(I, case):
    S, B, H, W, E, K, c0, extra = case
    coarse = torch.full((B, I["h"], I["w"], c0 + E + extra), 123.0)
    coarse[..., c0:c0 + E] = torch.from_numpy(I["coarse"])
    return coarse.cuda()


# ----------------------------------------------------------------------------------------------- 1. kernel vs materialised chain
@pytest.mark.parametrize("case,variant", PAIRS, ids=lambda p: "s%d_B%d_%dx%d_E%d_K%d" % p[:6] if len(p) == 8 else "%s_T%g_w%g" % p)
def test_kernel_vs_materialised_chain(case, variant):
    """Measured on an MI355X (worst over the pairs): see DESIGN.md 7p."""
    S, B, H, W, E, K, c0, extra = case
    kind, T, weight = variant
    I = Bh.inputs(case, kind, synth, G)
    crop, h, w, seed, exclude, uset, tnp, emb_np = I["crop"], I["h"], I["w"], I["seed"], I["exclude"], I["unseen"], I["target"], I["emb"]
    assert crop == (models.CROP if S == 32 else models.CROP_UP8) and (tnp == HIDDEN).any()
    ldc = c0 + E + extra
    emb = cu(emb_np)
    t = cu(tnp)
    st = L.stream_ptr()
    unseen = [k for k in range(K) if k % 3 == 1]    # the grouping of modes 1 / 2: another set than `exclude` and the bias set
    gmap = cu((np.random.RandomState(seed + 2).rand(B, H, W) < 0.5).astype(np.int64))
    coarse = _padded(I, case)
    # the materialised chain: upsample on the GPU, the loss and its gradient in float64 on the host, the transposed upsample on the GPU
    score = torch.empty(B, E, H, W, device="cuda")
    L.call("szn_bilinear_up_crop_fwd", S, B, h, w, E, ldc, c0, H, W, crop, L.ptr(coarse), L.ptr(score), st)
    torch.cuda.synchronize()
    score_np = score.cpu().numpy()
    oloss, ods, ostats = Bh.bias_ref(score_np, tnp, emb_np, exclude, T, uset, weight, HIDDEN)
    dscore = cu(ods.astype(np.float32))
    rdc = torch.zeros(B, h, w, ldc, device="cuda")
    L.call("szn_bilinear_up_crop_bwd", S, B, h, w, E, ldc, c0, H, W, crop, L.ptr(dscore), L.ptr(rdc), st)
    # the fused head
    kw = dict(exclude=exclude, T=T, bias=(uset, weight, HIDDEN))
    loss, stats, pred, dc = _head(FN, S, coarse, emb, H, W, c0, t, dtype=torch.float32, **kw)
    torch.cuda.synchronize()
    eloss = abs(float(loss) - oloss) / abs(oloss)
    estats = rel(stats[:, 0], ostats[:, 0])
    egrad = rel(dc[..., c0:c0 + E], rdc[..., c0:c0 + E])
    pu = Bh.unseen_prob(score_np, emb_np, T, uset)[tnp == HIDDEN]
    print("%s %s: loss %.9g reference %.9g rel err %.3e; stats err %.3e; d(coarse) err / max %.3e; hidden px %d, median P_U %.3g"
          % (case, variant, float(loss), oloss, eloss, estats, egrad, int((tnp == HIDDEN).sum()), float(np.median(pu))))
    assert np.isfinite(float(loss)) and bool(torch.isfinite(dc[..., c0:c0 + E]).all())
    counted = ((tnp >= 0) & (tnp < K) & ~np.isin(tnp, exclude)) | (tnp == HIDDEN)
    assert np.array_equal(stats[:, 1].cpu().numpy(), ostats[:, 1]) and np.array_equal(ostats[:, 1], counted.sum(axis=(1, 2)))     # exact
    assert eloss < 1e-3, (float(loss), oloss)
    assert estats < 1e-3
    assert egrad < 1e-4
    assert bool((dc[..., :c0] == SENT).all()) and bool((dc[..., c0 + E:] == SENT).all())
    # pred: the cosine fused head's, bit for bit, in the three group modes; the loss does not depend on the group
    for mode in (0, 1, 2):
        gk = dict(target=t, unseen=unseen if mode else None, mode=mode, gmap=gmap if mode == 1 else None)
        ps = _head(FN, S, coarse, emb, H, W, c0, **gk, **kw)
        pc = _head("szn_fused_head_grouped", S, coarse, emb, H, W, c0, **gk)
        assert torch.equal(ps[2], pc[2]), mode
        assert same_bits(ps[0], loss) and same_bits(ps[1], stats), mode
        if mode == 0:
            assert torch.equal(ps[2], pred)
    p_only = _head(FN, S, coarse, emb, H, W, c0, **kw)[2]                      # pred-only: no target, no softmax
    assert torch.equal(p_only, pred)
    # 16-bit d(coarse): the fp32 result rounded to the type, to within 1 ulp (the store may round the scaled sum once); padding untouched
    for dt in (torch.bfloat16, torch.float16):
        _, _, p16, d16 = _head(FN, S, coarse, emb, H, W, c0, t, want_pred=False, dtype=dt, **kw)        # loss-only + dcoarse
        assert p16 is None
        want = dc[..., c0:c0 + E].to(dt)
        ulps = (_ordered16(d16[..., c0:c0 + E]) - _ordered16(want)).abs().max()
        assert int(ulps) <= 1, (dt, int(ulps))
        assert bool((d16[..., :c0] == SENT).all()) and bool((d16[..., c0 + E:] == SENT).all())
    # loss-only (no pred, no dcoarse), prepared == unprepared, and a second full call: the same bits
    l2, s2, _, _ = _head(FN, S, coarse, emb, H, W, c0, t, want_pred=False, **kw)
    ws = torch.empty(L.load().szn_fused_head_workspace_bytes(B, h, w, E, K), dtype=torch.uint8, device="cuda")
    L.call("szn_fused_head_prepare", E, K, L.ptr(emb), L.ptr(ws), st)
    outs = [_head(FN, S, coarse, emb, H, W, c0, t, dtype=torch.float32, ws=ws, **kw) for _ in range(2)]
    outs.append(_head(FN, S, coarse, emb, H, W, c0, t, dtype=torch.float32, **kw))
    torch.cuda.synchronize()
    assert same_bits(l2, loss) and same_bits(s2, stats)
    for o in outs:
        assert same_bits(o[0], loss) and same_bits(o[1], stats) and torch.equal(o[2], pred) and same_bits(o[3], dc)


# ----------------------------------------------------------------------------------------------- 2. no hidden pixel: sim_ce's bits
@pytest.mark.parametrize("case", [R.CASES[0], R.CASES[3], R.CASES[4]], ids=lambda c: "s%d_B%d_%dx%d_E%d_K%d" % c[:6])
def test_without_hidden_pixels_every_output_is_sim_ce_bit_for_bit(case):
    S, B, H, W, E, K, c0, extra = case
    I = Bh.inputs(case, "uniform", synth, G)
    tnp = np.where(I["target"] == HIDDEN, -1, I["target"])
    t, emb, coarse = cu(tnp), cu(I["emb"]), _padded(I, case)
    unseen = [k for k in range(K) if k % 3 == 1]
    gmap = cu((np.random.RandomState(I["seed"] + 2).rand(B, H, W) < 0.5).astype(np.int64))
    kw = dict(exclude=I["exclude"], T=0.1)
    for mode in (0, 1, 2):
        gk = dict(target=t, unseen=unseen if mode else None, mode=mode, gmap=gmap if mode == 1 else None)
        for dt in (torch.float32, torch.bfloat16, torch.float16):
            a = _head(FN, S, coarse, emb, H, W, c0, dtype=dt, bias=(I["unseen"], 2.0, HIDDEN), **gk, **kw)
            b = _head("szn_fused_simce_head", S, coarse, emb, H, W, c0, dtype=dt, **gk, **kw)
            torch.cuda.synchronize()
            assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and torch.equal(a[2], b[2]) and same_bits(a[3], b[3]), (mode, dt)
    # and a hidden pixel does change them (the comparison above is not vacuous)
    c = _head(FN, S, coarse, emb, H, W, c0, cu(I["target"]), dtype=torch.float32, bias=(I["unseen"], 2.0, HIDDEN), **kw)
    assert not same_bits(c[0], b[0]) and float(c[1][:, 1].sum()) > float(b[1][:, 1].sum())


# ----------------------------------------------------------------------------------------------- 3. argument errors
@pytest.mark.parametrize("prepared", [False, True])
def test_argument_errors_launch_nothing(prepared):
    S, B, H, W, E, K = 32, 1, 40, 40, 20, 21
    crop = models.CROP
    h, w = (H + crop + S - 1) // S, (W + crop + S - 1) // S
    emb = cu(R.embeddings(K, E, synth, G))
    coarse = cu(synth.uniform(3, (B, h, w, E), -2, 2))
    t = cu(Bh.hide(R.labels(B, H, W, K, [0], 4), 0.2, 5))
    fn = FN + ("_prepared" if prepared else "")
    lib = L.load()
    U = [2, 5]
    bad = [(None, 0.1, (None, 1.0, HIDDEN), "bias set"), (None, 0.1, (list(range(K)), 1.0, HIDDEN), "bias set"),
           (None, 0.1, ([K], 1.0, HIDDEN), "bias set"), (None, 0.1, ([1, 255], 1.0, HIDDEN), "bias set"),
           (None, 0.1, (U, 0.0, HIDDEN), "weight"), (None, 0.1, (U, -2.0, HIDDEN), "weight"),
           (None, 0.1, (U, float("nan"), HIDDEN), "weight"), (None, 0.1, (U, float("inf"), HIDDEN), "weight"),
           (None, 0.1, (U, 1.0, -1), "hidden label"), (None, 0.1, (U, 1.0, 0), "hidden label"), (None, 0.1, (U, 1.0, 7), "hidden label"),
           (None, 0.0, (U, 1.0, HIDDEN), "temperature"), (None, float("nan"), (U, 1.0, HIDDEN), "temperature"),
           (list(range(K)), 0.1, (U, 1.0, HIDDEN), "competing"), ([K], 0.1, (U, 1.0, HIDDEN), "exclude")]
    for exclude, T, bias, word in bad:
        loss, stats = torch.full((1,), SENT, device="cuda"), torch.full((B, 2), SENT, device="cuda")
        pred = torch.full((B, H, W), -7, dtype=torch.int64, device="cuda")
        dc = torch.full((B, h, w, E), SENT, device="cuda")
        ws = torch.full((lib.szn_fused_head_workspace_bytes(B, h, w, E, K),), 0x5A, dtype=torch.uint8, device="cuda")
        a = _args(fn, S, coarse, emb, H, W, 0, t, None, 0, None, exclude, T, bias, loss, stats, pred, dc, ws)
        rc = getattr(lib, a[0])(*a[1:])
        assert rc == -1, (exclude, T, bias, rc)                              # SZN_ERR_ARG
        assert word in lib.szn_last_error().decode(), lib.szn_last_error()
        torch.cuda.synchronize()
        assert bool((loss == SENT).all()) and bool((stats == SENT).all()) and bool((pred == -7).all()) and bool((dc == SENT).all())
        assert bool((ws == 0x5A).all())                                      # not even the embedding tables were written
