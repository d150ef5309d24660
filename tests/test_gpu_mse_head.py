"""GPU: the fused MSE embedding head (szn_fused_mse_head / _prepared) and train.py -loss mse on engine.TrainStep.

  1. the kernel against the materialised chain szn_bilinear_up_crop_fwd -> szn_mse_loss_fwd -> szn_embed_argmax_k -> szn_mse_loss_bwd ->
     szn_bilinear_up_crop_bwd on the same coarse map: pred bit-equal to the cosine fused head's in group modes 0 / 1 / 2, counts exact,
     d(coarse) within 1e-4 of the chain's (relative to its max), loss within 1e-3 of oracle.mse_loss on the materialised score for a
     uniform random map and two near-converged ones (C = e_label + r |e| noise, r = 1e-2 and 1e-3: the inputs on which the expanded
     form |s|^2 - 2 s.e + |e|^2 loses the loss), 16-bit d(coarse), untouched padding, pred-only / loss-only calls, prepared ==
     unprepared, two runs bit-identical;
  1b. the loss on inputs whose every valid pixel is converged (|s - e|^2 <= r^2 |e|^2): batch, image and single-cell sums within 1e-3
     of the oracle, and a CPU restatement of the expanded form shown to miss that gate on the same inputs;
  2. the full fp32 step against the CPU oracle (backward given the HIP forward state, tests/helpers_parity.py);
  3. TrainStep(loss="mse") against fused_head=False and the autograd route (FCN32s), FCN8s against its autograd route;
  4. fp16 with the dynamic loss scale, next to the cosine step on the same batch;
  5. the trainer and the CLI (bf16, fp16) with validation on the fused route: plain, test_all and forced unseen;
  6. two data-parallel ranks on one GPU against one process with both images (fused Adam, sharded optimizer once).

Measured on an MI355X (relative loss error vs the oracle on the materialised score, worst case of CASES): see DESIGN.md section 7e.
"""
import glob
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import szn_oracle as O  # noqa: E402
from helpers_parity import adopt_forward  # noqa: E402
from zeroshotsemanticsegmentation_amd import _lib as L  # noqa: E402
from zeroshotsemanticsegmentation_amd import engine, models, optim, synth, train, trainer_fcn, utils  # noqa: E402
from zeroshotsemanticsegmentation_amd.synthetic_dataset import SyntheticSegmentation  # noqa: E402

G = os.path.join(ROOT, "tests", "golden")
SENT = -7.25          # sentinel of the channels outside [c0, c0 + E)


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
    """the Context embeddings where the repository has them for this E (first K rows), the synthetic recipe otherwise"""
    path = os.path.join(G, "embeddings_context_%d.npy" % E)
    if os.path.exists(path):
        e = np.load(path).astype(np.float32)
        if e.shape[0] >= K:
            return np.ascontiguousarray(e[:K])
    return synth.make_embeddings(K, E, seed=5)


# ----------------------------------------------------------------------------------------------- 1. kernel vs materialised chain
def _head(fn, S, coarse, emb, H, W, c0, target=None, unseen=None, mode=0, gmap=None, want_pred=True, dtype=None, ws=None):
    """one call of szn_fused_mse_head / szn_fused_head_grouped (+ _prepared when `ws` holds the tables) -> loss, stats, pred, dcoarse"""
    B, h, w, ldc = coarse.shape
    K, E = emb.shape
    crop = models.CROP if S == 32 else models.CROP_UP8
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
    L.call(fn, S, B, h, w, E, ldc, c0, H, W, crop, K, L.ptr(coarse), L.ptr(emb), L.ptr(target), L.class_set(unseen), mode, L.ptr(gmap),
           L.ptr(loss), L.ptr(stats), L.ptr(pred), L.dtype_code(dtype) if dc is not None else 0, L.ptr(dc), L.ptr(ws), L.stream_ptr())
    return loss, stats, pred, dc


def _labels(B, H, W, K, seed, block):
    t = synth.make_labels(B, H, W, K, seed=seed, block=block, ignore_frac=0.06)
    r = np.random.RandomState(seed).rand(B, H, W)
    t[r < 0.03] = -2                                # batch padding
    t[(r >= 0.03) & (r < 0.05)] = K + 1             # out of range: row 0 (szn_mse_loss_fwd's contract)
    return t


def _maps(S, B, h, w, E, H, W, crop, emb, target, seed):
    """the three coarse maps of the loss check: uniform [-2, 2], and e_label(position) + r |e| noise for r = 1e-2, 1e-3"""
    out = [("uniform", synth.uniform(seed, (B, h, w, E), -2, 2))]
    yy = np.clip(S * np.arange(h) + S // 2 - crop, 0, H - 1)
    xx = np.clip(S * np.arange(w) + S // 2 - crop, 0, W - 1)
    lab = target[:, yy][:, :, xx]
    lab = np.where((lab < 0) | (lab >= emb.shape[0]), 0, lab)
    base = emb[lab]                                                       # (B,h,w,E)
    nrm = np.linalg.norm(base, axis=-1, keepdims=True)
    noise = np.random.RandomState(seed + 7).randn(B, h, w, E).astype(np.float32)
    for r in (1e-2, 1e-3):
        out.append(("r=%g" % r, (base + np.float32(r) * nrm * noise).astype(np.float32)))
    return out


CASES = [  # stride, B, H, W, E, K, c0, padding channels behind, label block
    (32, 2, 70, 101, 20, 33, 0, 42, 8),           # the shapes of test_fused_head_matches_unfused ...
    (32, 1, 512, 512, 300, 21, 0, 20, 64),
    (32, 1, 1, 1, 20, 21, 0, 44, 8),
    (32, 2, 32, 32, 20, 59, 0, 44, 8),
    (32, 2, 97, 131, 300, 59, 3, 1, 48),          # ... a channel offset, and K = 59 at E = 300 with single-label and mixed cells
    (8, 3, 33, 47, 20, 150, 0, 12, 8),            # stride 8 (FCN8s)
    (8, 1, 97, 131, 300, 59, 2, 2, 24),
    (8, 2, 64, 64, 20, 256, 0, 0, 4),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "s%d_B%d_%dx%d_E%d_K%d" % c[:6])
def test_kernel_vs_materialised_chain(case):
    S, B, H, W, E, K, c0, extra, block = case
    crop = models.CROP if S == 32 else models.CROP_UP8
    h, w = (H + crop + S - 1) // S, (W + crop + S - 1) // S
    ldc = c0 + E + extra
    seed = S * 1000 + E + K
    emb_np = _emb(K, E)
    emb = cu(emb_np)
    tnp = _labels(B, H, W, K, seed + 1, block)
    t = cu(tnp)
    st = L.stream_ptr()
    unseen = [k for k in range(K) if k % 3 == 1]
    gmap = cu((np.random.RandomState(seed + 2).rand(B, H, W) < 0.5).astype(np.int64))
    for name, cmap in _maps(S, B, h, w, E, H, W, crop, emb_np, tnp, seed):
        coarse = torch.full((B, h, w, ldc), 123.0)
        coarse[..., c0:c0 + E] = torch.from_numpy(cmap)
        coarse = coarse.cuda()
        # the materialised chain
        score = torch.empty(B, E, H, W, device="cuda")
        L.call("szn_bilinear_up_crop_fwd", S, B, h, w, E, ldc, c0, H, W, crop, L.ptr(coarse), L.ptr(score), st)
        lws = torch.empty(L.load().szn_loss_workspace_bytes(B, H, W), dtype=torch.uint8, device="cuda")
        rloss, rstats = torch.empty(1, device="cuda"), torch.empty(B, 2, device="cuda")
        L.call("szn_mse_loss_fwd", B, E, H, W, K, L.ptr(score), L.ptr(t), L.ptr(emb), None, L.ptr(rloss), L.ptr(rstats), L.ptr(lws), st)
        dscore = torch.empty_like(score)
        L.call("szn_mse_loss_bwd", B, E, H, W, K, L.ptr(score), L.ptr(t), L.ptr(emb), None, L.ptr(rstats), None, L.ptr(dscore), st)
        rdc = torch.zeros(B, h, w, ldc, device="cuda")
        L.call("szn_bilinear_up_crop_bwd", S, B, h, w, E, ldc, c0, H, W, crop, L.ptr(dscore), L.ptr(rdc), st)
        torch.cuda.synchronize()
        oloss, _, ostats = O.mse_loss(score.cpu().numpy(), tnp, embed=emb_np, want_grad=False)
        del score, dscore
        # the fused head
        loss, stats, pred, dc = _head("szn_fused_mse_head", S, coarse, emb, H, W, c0, t, dtype=torch.float32)
        torch.cuda.synchronize()
        eloss = abs(float(loss) - float(oloss)) / abs(float(oloss))
        print("%s %s: loss %.9g oracle %.9g rel err %.3e (chain kernel %.3e); d(coarse) rel err %.3e"
              % (case, name, float(loss), float(oloss), eloss, abs(float(rloss) - float(oloss)) / abs(float(oloss)),
                 rel(dc[..., c0:c0 + E], rdc[..., c0:c0 + E])))
        assert eloss < 1e-3, (name, float(loss), float(oloss))
        assert rel(stats[:, 0], ostats[:, 0]) < 1e-3, name
        assert torch.equal(stats[:, 1], rstats[:, 1]) and np.array_equal(stats[:, 1].cpu().numpy(), ostats[:, 1])     # counts: exact
        assert int(stats[:, 1].sum()) == int((tnp >= 0).sum())
        assert rel(dc[..., c0:c0 + E], rdc[..., c0:c0 + E]) < 1e-4, name
        assert bool((dc[..., :c0] == SENT).all()) and bool((dc[..., c0 + E:] == SENT).all())
        # pred: the cosine fused head's, bit for bit, in the three group modes (mode 0 also pred-only)
        for mode in (0, 1, 2):
            kw = dict(target=t, unseen=unseen if mode else None, mode=mode, gmap=gmap if mode == 1 else None)
            pm = _head("szn_fused_mse_head", S, coarse, emb, H, W, c0, **kw)
            pc = _head("szn_fused_head_grouped", S, coarse, emb, H, W, c0, **kw)
            assert torch.equal(pm[2], pc[2]), (name, mode)
            assert same_bits(pm[0], loss) and same_bits(pm[1], stats), (name, mode)        # the loss does not depend on the group
            if mode == 0:
                assert torch.equal(pm[2], pred)
        p_only = _head("szn_fused_mse_head", S, coarse, emb, H, W, c0)[2]
        assert torch.equal(p_only, pred)
        # 16-bit d(coarse): the rounding of the fp32 result (IEEE round-to-nearest-even, taken on the CPU); padding untouched
        for dt in (torch.bfloat16, torch.float16):
            _, _, p16, d16 = _head("szn_fused_mse_head", S, coarse, emb, H, W, c0, t, want_pred=False, dtype=dt)     # loss-only + dcoarse
            assert p16 is None
            want = dc[..., c0:c0 + E].cpu().to(dt)
            assert torch.equal(d16[..., c0:c0 + E].cpu().view(torch.int16), want.view(torch.int16)), (name, dt)
            assert bool((d16[..., :c0] == SENT).all()) and bool((d16[..., c0 + E:] == SENT).all())
        # loss-only (no pred, no dcoarse), prepared == unprepared, and a second full call: the same bits
        l2, s2, _, _ = _head("szn_fused_mse_head", S, coarse, emb, H, W, c0, t, want_pred=False)
        ws = torch.empty(L.load().szn_fused_head_workspace_bytes(B, h, w, E, K), dtype=torch.uint8, device="cuda")
        L.call("szn_fused_head_prepare", E, K, L.ptr(emb), L.ptr(ws), st)
        outs = [_head("szn_fused_mse_head", S, coarse, emb, H, W, c0, t, dtype=torch.float32, ws=ws) for _ in range(2)]
        outs.append(_head("szn_fused_mse_head", S, coarse, emb, H, W, c0, t, dtype=torch.float32))
        torch.cuda.synchronize()
        assert same_bits(l2, loss) and same_bits(s2, stats)
        for o in outs:
            assert same_bits(o[0], loss) and same_bits(o[1], stats) and torch.equal(o[2], pred) and same_bits(o[3], dc), name


# ----------------------------------------------------------------------------------------------- 1b. the loss where it IS small
# The maps of section 1 are near-converged position by position, but their labels are not (mixed-class cells, -2 / K+1 labels, missing
# border taps), so their total loss stays of order |e|^2 and cannot tell a cancelling formula from a sound one.  Here every valid pixel
# is converged: the coarse class map is constant over 3 x 3 positions (image 0: one class), C = e_class + r |e| n with |n| = 1, and a
# pixel is labelled (with that class) only where all four taps of its cell exist and carry it -- so |s - e|^2 <= r^2 |e|^2 on every
# valid pixel.  The same gate (1e-3 against oracle.mse_loss on the materialised score) then holds for the batch loss, for each image's
# sum and for single cells.  _expanded_fp32 restates the tempting per-cell form |s|^2 - 2 s.e + |e|^2 from fp32 G / Q tables on the
# CPU: the test asserts that THAT form misses the gate on these inputs at r = 1e-3, i.e. that the inputs can tell.
def _bil(S, t):
    return 1.0 - np.abs(t - (S - 0.5)) / S


def _converged_input(S, B, h, w, E, H, W, crop, emb, r, seed):
    K = emb.shape[0]
    rs = np.random.RandomState(seed)
    clab = rs.randint(0, K, size=(B, (h + 2) // 3, (w + 2) // 3)).repeat(3, axis=1).repeat(3, axis=2)[:, :h, :w].copy()
    clab[0] = rs.randint(K)
    n = rs.randn(B, h, w, E)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    base = emb[clab].astype(np.float64)
    C = (base + r * np.linalg.norm(base, axis=-1, keepdims=True) * n).astype(np.float32)
    I, J = (np.arange(H) + crop) // S, (np.arange(W) + crop) // S
    okI, okJ = (I >= 1) & (I <= h - 1), (J >= 1) & (J <= w - 1)
    Ic, Jc = np.clip(I, 1, h - 1), np.clip(J, 1, w - 1)
    taps = [clab[:, Ic - 1 + a][:, :, Jc - 1 + b] for a in (0, 1) for b in (0, 1)]
    same = (taps[0] == taps[1]) & (taps[0] == taps[2]) & (taps[0] == taps[3]) & okI[None, :, None] & okJ[None, None, :]
    target = np.where(same, taps[0], -1).astype(np.int64)
    return C, target


def _per_pixel(S, C, emb, target, crop):
    """for the valid pixels of a _converged_input: (image, cell id, |s - e|^2 in float64, the expanded per-cell form in fp32)"""
    B, h, w, E = C.shape
    H, W = target.shape[1:]
    Y, X = np.arange(H) + crop, np.arange(W) + crop
    wy = np.stack([_bil(S, Y % S + S), _bil(S, Y % S)], 1)                  # weights of tap rows I - 1, I
    wx = np.stack([_bil(S, X % S + S), _bil(S, X % S)], 1)
    wt = (wy[:, None, :, None] * wx[None, :, None, :]).reshape(H, W, 4)      # exact in fp32: multiples of 1 / (2 S)^2
    T = np.stack([C[:, :-1, :-1], C[:, :-1, 1:], C[:, 1:, :-1], C[:, 1:, 1:]], axis=3)          # (B, h-1, w-1, 4, E): cell (I, J) at [I-1, J-1]
    Q32 = np.einsum("bijte,bijue->bijtu", T, T).astype(np.float32)
    G32 = np.einsum("bijte,ke->bijtk", T, emb).astype(np.float32)
    en2 = np.einsum("ke,ke->k", emb, emb).astype(np.float32)
    b, y, x = np.nonzero(target >= 0)
    k = target[b, y, x]
    ci, cj = Y[y] // S - 1, X[x] // S - 1
    wp = wt[y, x]                                                            # (n, 4)
    tp = T[b, ci, cj].astype(np.float64)                                     # (n, 4, E)
    d = np.einsum("nt,nte->ne", wp, tp) - emb[k].astype(np.float64)
    ref = np.einsum("ne,ne->n", d, d)
    w32 = wp.astype(np.float32)
    ss = np.einsum("nt,nu,ntu->n", w32, w32, Q32[b, ci, cj]).astype(np.float32)
    se = np.einsum("nt,nt->n", w32, G32[b, ci, cj, :, k]).astype(np.float32)
    exp32 = (ss - np.float32(2) * se).astype(np.float32) + en2[k]
    cell = (b * (h - 1) + ci) * (w - 1) + cj
    return b, cell, ref, exp32.astype(np.float64)


CONVERGED = [  # stride, B, H, W, E, K
    (32, 2, 97, 131, 300, 59),
    (32, 2, 70, 101, 20, 33),
    (8, 2, 97, 131, 300, 59),
    (8, 2, 33, 47, 20, 33),
]


@pytest.mark.parametrize("case", CONVERGED, ids=lambda c: "s%d_B%d_%dx%d_E%d_K%d" % c)
@pytest.mark.parametrize("r", [1e-2, 1e-3])
def test_loss_on_converged_pixels(case, r):
    """Measured on an MI355X: fused head <= 3.7e-6 on every batch, image and cell sum; the expanded fp32 form at
    r = 1e-3: 6e-3 .. 2.2e-1 per image, median 1e-1 .. 2.6e-1 per cell."""
    S, B, H, W, E, K = case
    crop = models.CROP if S == 32 else models.CROP_UP8
    h, w = (H + crop + S - 1) // S, (W + crop + S - 1) // S
    emb_np = _emb(K, E)
    Cnp, tnp = _converged_input(S, B, h, w, E, H, W, crop, emb_np, r, seed=S + E)
    assert all((tnp[i] >= 0).sum() >= 16 for i in range(B))
    img, cell, ref, exp32 = _per_pixel(S, Cnp, emb_np, tnp, crop)
    assert ref.max() <= 1.0001 * (r * np.linalg.norm(emb_np, axis=1).max()) ** 2          # every valid pixel is converged
    coarse, emb = cu(Cnp), cu(emb_np)
    st = L.stream_ptr()
    score = torch.empty(B, E, H, W, device="cuda")
    L.call("szn_bilinear_up_crop_fwd", S, B, h, w, E, E, 0, H, W, crop, L.ptr(coarse), L.ptr(score), st)
    torch.cuda.synchronize()
    score_np = score.cpu().numpy()

    def both(target):
        oloss, _, ostats = O.mse_loss(score_np, target, embed=emb_np, want_grad=False)
        loss, stats, _, _ = _head("szn_fused_mse_head", S, coarse, emb, H, W, 0, cu(target), want_pred=False)
        torch.cuda.synchronize()
        assert np.array_equal(stats[:, 1].cpu().numpy(), ostats[:, 1])
        return float(loss), float(oloss), stats[:, 0].double().cpu().numpy(), ostats[:, 0].astype(np.float64)

    loss, oloss, s, os_ = both(tnp)
    e_img = np.abs(s - os_) / os_
    # the CPU restatement of the expanded form, per image and per cell, against the float64 per-pixel reference
    x_img = np.array([abs(exp32[img == i].sum() - ref[img == i].sum()) / ref[img == i].sum() for i in range(B)])
    cells = np.unique(cell)
    rc = np.array([ref[cell == c].sum() for c in cells])
    x_cell = np.abs(np.array([exp32[cell == c].sum() for c in cells]) - rc) / rc
    assert np.allclose([ref[img == i].sum() for i in range(B)], os_, rtol=1e-4)           # the reference of the restatement = the oracle's
    print("%s r=%g: loss %.6e oracle %.6e rel err %.2e; per image %s | expanded fp32 form: per image %s, per cell median %.2e max %.2e"
          % (case, r, loss, oloss, abs(loss - oloss) / oloss, ["%.2e" % v for v in e_img], ["%.2e" % v for v in x_img],
             np.median(x_cell), x_cell.max()))
    assert abs(loss - oloss) < 1e-3 * oloss, (loss, oloss)
    assert e_img.max() < 1e-3, e_img
    # single cells: the three on which the expanded form is worst
    worst = cells[np.argsort(x_cell)[-3:]]
    for c in worst:
        t1 = np.full_like(tnp, -1)
        bb, yy, xx = np.nonzero(tnp >= 0)
        pick = cell == c
        t1[bb[pick], yy[pick], xx[pick]] = tnp[bb[pick], yy[pick], xx[pick]]
        b0 = int(bb[pick][0])
        _, _, s1, o1 = both(t1)
        e1 = abs(s1[b0] - o1[b0]) / o1[b0]
        print("   cell %d (image %d, %d px): fused rel err %.2e" % (c, b0, int(pick.sum()), e1))
        assert e1 < 1e-3, (c, e1)
    if r == 1e-3:
        assert x_cell.max() > 1e-3 and np.median(x_cell) > 1e-3, "these inputs would not catch the expanded form"


# ----------------------------------------------------------------------------------------------- 2. full step vs the oracle
E2, K2, H2 = 20, 33, 256


def _oracle_params(m):
    return {k: v.detach().cpu().numpy() for k, v in m.named_parameters() if k.split(".")[0] != "upscore"}


def test_train_step_vs_oracle():
    """one fp32 TrainStep(loss="mse") at 256 x 256, E = 20, K = 33 against the CPU oracle: loss against its own forward pass; every
    parameter gradient against its backward from O.mse_loss's gradient on the HIP forward state (1e-4 weights, 1e-3 biases)"""
    emb = _emb(K2, E2)
    m = models.FCN32s(E2).load_synthetic(1337, device=torch.device("cuda")).eval()
    x = synth.make_images(1, H2, H2, seed=41)
    target = synth.make_labels(1, H2, H2, K2, seed=42)
    om = O.FCN32sOracle(_oracle_params(m), E2)
    ts = engine.TrainStep(m, emb, loss="mse", optimizer="adam", lr=1e-6, precision=torch.float32)
    ts.keep_ctx = True
    try:
        loss, pred = ts.step(cu(x), cu(target))
        torch.cuda.synchronize()
        ctx = ts.last_ctx
        of = om.forward(x, "fcn")
        oloss, _, _ = O.mse_loss(of, target, embed=emb, want_grad=False)
        assert abs(float(loss) - float(oloss)) < 1e-4 * abs(float(oloss)), (float(loss), float(oloss))
        sn = m._engine.upscore(ctx).cpu().numpy()
        hloss, ods, _ = O.mse_loss(sn, target, embed=emb)
        assert abs(float(loss) - float(hloss)) < 1e-5 * abs(float(hloss)), (float(loss), float(hloss))
        assert np.array_equal(pred.cpu().numpy(), utils.infer_lbl_device(cu(sn), cu(emb)).cpu().numpy())
        assert adopt_forward(om, ctx, x, None, E2) == 0.0
        og = om.backward(df=ods)
        og = {k: v for k, v in og.items() if k.split(".")[0] in O.WEIGHT_GROUP}
        assert len(og) >= 32
        for k, r in og.items():
            name, kind = k.split(".")
            e = rel(getattr(getattr(m, name), kind).grad, r)
            assert e < (1e-3 if kind == "bias" else 1e-4), (k, e)
    finally:
        ts.last_ctx = None


# ----------------------------------------------------------------------------------------------- 3. TrainStep vs the other routes
def _grad_rel(ma, mb, names):
    out = {}
    for n in names:
        for kind in ("weight", "bias"):
            out["%s.%s" % (n, kind)] = rel(getattr(getattr(mb, n), kind).grad, getattr(getattr(ma, n), kind).grad)
    return out


def _sgd(m, emb, **kw):
    return engine.TrainStep(m, emb, loss="mse", optimizer="sgd", lr=1e-6, momentum=0.99, weight_decay=0.0005, precision=torch.float32, **kw)


def _torch_sgd(m):
    layers = models.opt_layers(m)
    return torch.optim.SGD([{"params": [getattr(m, n).weight for n in layers]},
                            {"params": [getattr(m, n).bias for n in layers], "lr": 2e-6, "weight_decay": 0.0}],
                           lr=1e-6, momentum=0.99, weight_decay=0.0005)


def test_train_step_equals_unfused_head_and_autograd_route():
    H, B = 256, 2
    dev = torch.device("cuda")
    emb = _emb(K2, E2)
    x = cu(synth.make_images(B, H, H, seed=43))
    t = cu(synth.make_labels(B, H, H, K2, seed=44))
    ma = models.FCN32s(E2).load_synthetic(1337, device=dev).eval()
    opt = _torch_sgd(ma)
    mb = models.FCN32s(E2).load_synthetic(1337, device=dev).eval()
    mc = models.FCN32s(E2).load_synthetic(1337, device=dev).eval()
    tb, tc = _sgd(mb, emb), _sgd(mc, emb, fused_head=False)
    for it in range(2):
        score = ma(x, mode="fcn")
        loss = utils.mse_loss(score, t, cu(emb))
        apred = utils.infer_lbl_device(score.detach(), cu(emb))
        opt.zero_grad()
        loss.backward()
        opt.step()
        lb, pb = tb.step(x, t)
        lc, pc = tc.step(x, t)
        torch.cuda.synchronize()
        assert torch.equal(pc, apred)
        assert float((pb != apred).float().mean()) < 2e-3              # the algebraic head may flip exact near-ties only
        assert abs(float(lb) - float(loss)) < 1e-6 * abs(float(loss)) and abs(float(lc) - float(loss)) < 1e-6 * abs(float(loss))
        for mm in (mb, mc):
            if it == 0:             # gradients on the same forward state (afterwards ReLU / pooling flips: tests/helpers_parity.py)
                for k, e in _grad_rel(ma, mm, models._OPT_LAYERS).items():
                    assert e < 1e-4, (k, it, e)
            for (na, pa), (nb, pb_) in zip(ma.named_parameters(), mm.named_parameters()):
                assert na == nb
                if na.split(".")[0] in models._OPT_LAYERS:
                    assert rel(pb_, pa) < (1e-5 if it == 0 else 2e-4), (na, it)


def test_fcn8s_train_step_vs_autograd():
    H, B = 256, 1
    dev = torch.device("cuda")
    emb = _emb(K2, E2)
    x = cu(synth.make_images(B, H, H, seed=45))
    t = cu(synth.make_labels(B, H, H, K2, seed=46))
    ma = models.FCN8s(E2).load_synthetic(1337, device=dev).eval()
    mb = models.FCN8s(E2).load_synthetic(1337, device=dev).eval()
    md = models.FCN8s(E2).load_synthetic(1337, device=dev).eval()
    score = ma(x, mode="fcn")
    loss = utils.mse_loss(score, t, cu(emb))
    loss.backward()
    lb, pb = _sgd(mb, emb).step(x, t)
    ld, pd = md.embed_loss(x, emb, t, loss="mse")                      # the autograd bridge with the fused stride-8 head
    ld.backward()
    torch.cuda.synchronize()
    assert float((pb != utils.infer_lbl_device(score.detach(), cu(emb))).float().mean()) < 2e-3 and torch.equal(pb, pd)
    assert abs(float(lb) - float(loss)) < 1e-6 * abs(float(loss)) and abs(float(ld) - float(loss)) < 1e-6 * abs(float(loss))
    for mm in (mb, md):
        for k, e in _grad_rel(ma, mm, models.opt_layers(mb)).items():
            assert e < 1e-5, (k, e)
    # inference: embed_predict(loss="mse") gives the step's kind of loss and the cosine route's prediction
    with torch.no_grad():
        l2, p2 = ma.embed_predict(x, emb, t, loss="mse")
        _, p3 = ma.embed_predict(x, emb, t)
        ref = float(utils.mse_loss(ma(x, mode="fcn"), t, cu(emb)))
    assert torch.equal(p2, p3) and abs(float(l2) - ref) < 1e-6 * abs(ref)


# ----------------------------------------------------------------------------------------------- 4. fp16
def test_fp16_mse_steps():
    """a few fp16 steps: finite losses, the dynamic loss scale's state (applied steps, scale relative to its start: cosine 4096,
    mse 512 -- engine.TrainStep says why) moves exactly as the cosine step's on the same batch"""
    H, B = 96, 2
    emb = synth.make_embeddings(K2, E2)
    x = cu(synth.make_images(B, H, H, seed=71))
    t = cu(synth.make_labels(B, H, H, K2, seed=72, block=16))
    state = {}
    for kind in ("cos", "mse"):
        m = models.FCN32s(E2).load_synthetic(1337, device=torch.device("cuda")).eval()
        ts = engine.TrainStep(m, emb, loss=kind, optimizer="adam", lr=1e-5, precision=torch.float16)
        scale0 = ts.loss_scale
        assert ts.dynamic and scale0 == (4096.0 if kind == "cos" else 512.0)
        losses = [float(ts.step(x, t)[0]) for _ in range(4)]
        torch.cuda.synchronize()
        assert all(np.isfinite(losses)), (kind, losses)
        state[kind] = (ts.applied_steps, ts.loss_scale / scale0, losses)
        g = m.score_fr.weight.grad.detach().float() / ts.loss_scale
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    print("fp16 state (applied steps, scale, losses):", state)
    assert state["mse"][:2] == state["cos"][:2], state               # no skipped step unless the cosine step skips there too
    assert state["mse"][2][-1] < state["mse"][2][0]                  # and it trains


# ----------------------------------------------------------------------------------------------- 5. trainer and CLI
E5, K5, H5, W5 = 20, 33, 48, 56
UNSEEN5, VAL_UNSEEN5 = [0, 12, 16, 18], [16, 18]


class _Record(object):
    def __init__(self, monkeypatch):
        self.names = []
        real = L.call

        def call(name, *a):
            self.names.append(name)
            return real(name, *a)
        monkeypatch.setattr(L, "call", call)

    def fused_mse(self):
        return any(n.startswith("szn_fused_mse_head") for n in self.names)

    def other_head(self):
        return any(n.startswith("szn_fused_head") and n != "szn_fused_head_prepare" for n in self.names)

    def materialised(self):
        return any(n in ("szn_bilinear_up32_crop_fwd", "szn_bilinear_up_crop_fwd", "szn_embed_argmax_k", "szn_mse_loss_fwd")
                   for n in self.names)


def _trainer(tmp, arch, forced):
    m = (models.FCN32s if arch == "fcn32s" else models.FCN8s)(E5)
    m.load_synthetic(1337, device=torch.device("cuda"))
    ds = SyntheticSegmentation(split="val", n_images=3, size=(H5, W5), n_class=K5, embed_dim=E5, seed=5)
    loader = torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False)
    layers = models.opt_layers(m)
    opt = optim.FusedAdam([{"params": [getattr(m, n).weight for n in layers]},
                           {"params": [getattr(m, n).bias for n in layers], "lr": 2e-5}], lr=1e-5)
    t = trainer_fcn.Trainer(cuda=True, model=m, optimizer=opt, train_loader=loader, val_loader=loader, log_dir=str(tmp),
                            dataset="context", max_epoch=1, tb_writer=None, pixel_embeddings=E5, loss_func="mse", unseen=UNSEEN5,
                            val_unseen=VAL_UNSEEN5, forced_unseen=forced)
    return m, loader, t


@pytest.mark.parametrize("arch,kind", [("fcn32s", "plain"), ("fcn32s", "szn"), ("fcn32s", "forced"), ("fcn8s", "szn")])
def test_validate_takes_fused_mse_route(fast_tmp, monkeypatch, arch, kind):
    m, loader, t = _trainer(fast_tmp, arch, forced=(kind == "forced"))
    step = t._fast_step()
    assert isinstance(step, engine.TrainStep) and step.loss_kind == "mse" and step.fused_head
    assert (step.forced_unseen is not None) == (kind == "forced")
    szn = kind == "szn"
    rec = _Record(monkeypatch)
    metrics = t.validate(both_fcn_and_seenmask=szn)
    assert rec.fused_mse() and not rec.materialised() and not rec.other_head(), rec.names
    new, old, lts = [], [], []
    with torch.no_grad():
        for data, target in loader:
            _, loss, pred, _ = t._predict_device(data, target, szn)
            new.append((float(loss), pred))
    rec.names.clear()
    t.verbose_val = True                 # forces the materialised route (it needs score.sum())
    with torch.no_grad():
        for data, target in loader:
            _, loss, pred, lt = t._predict_device(data, target, szn)
            old.append((float(loss), pred))
            lts.append(lt[0].cpu().numpy())
    assert rec.materialised() and not rec.fused_mse()
    for (la, pa), (lb, pb) in zip(new, old):
        assert torch.equal(pa, pb)
        assert abs(la - lb) <= 1e-5 * abs(lb), (la, lb)
    want = utils.label_accuracy_score(lts, [p[0].cpu().numpy() for _, p in old], K5, unseen=VAL_UNSEEN5)[0]
    np.testing.assert_allclose(np.array(metrics), np.array(want), rtol=1e-12, equal_nan=True)


def test_dense_target_embed_keeps_materialised_route(fast_tmp, monkeypatch):
    m, loader, t = _trainer(fast_tmp, "fcn32s", False)
    dense = []
    for data, target in loader:
        lbl = target[0] if isinstance(target, (tuple, list)) else target
        te = t.embeddings[lbl.clamp_min(0).cuda()].permute(0, 3, 1, 2).contiguous()
        dense.append((data, (lbl, te * (lbl.cuda() >= 0).unsqueeze(1).float())))
    t.val_loader = dense
    rec = _Record(monkeypatch)
    t.validate()
    assert rec.materialised() and not rec.fused_mse()


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_cli_mse_epoch(fast_tmp, monkeypatch, precision):
    rec = _Record(monkeypatch)
    name = "mse" + precision
    train.main(['-c', '4', '-loss', 'mse', '-ve', '1', '-tu', '1,13', '-vu', '17,19', '--precision', precision, '--synthetic', '2',
                '64', '64', '--workers', '0', '-dir', fast_tmp, '-n', name])
    log = glob.glob(os.path.join(fast_tmp, 'logs', name + '_CFG_4_*'))
    assert len(log) == 1 and 'FCN_LOSS_mse' in log[0]
    rows = open(os.path.join(log[0], 'train_log.csv')).read().strip().split('\n')
    losses = [float(r.split(',')[2]) for r in rows[1:]]
    assert len(losses) == 2 and all(np.isfinite(losses)), losses
    vrows = open(os.path.join(log[0], 'val_log.csv')).read().strip().split('\n')
    assert len(vrows) == 2 and np.isfinite(float(vrows[1].split(',')[2]))
    assert "szn_fused_mse_head_prepared" in rec.names and "szn_fused_mse_head" in rec.names        # the step, the validation
    assert not rec.materialised() and not rec.other_head(), sorted(set(rec.names))


# ----------------------------------------------------------------------------------------------- 6. data parallel
DP_H = 64          # the geometry of tests/test_gpu_ddp_single_gpu.py: B = 1 and B = 2 run the same kernels


def _dp_data():
    return synth.make_images(2, DP_H, DP_H, seed=63), synth.make_labels(2, DP_H, DP_H, K2, seed=64, block=16)


def _dp_worker(rank, world, port, q):
    try:
        import torch.distributed as dist
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        x, t = _dp_data()
        dev = torch.device("cuda", 0)
        emb = _emb(K2, E2)
        out = {"rank": rank}
        for sharded in (False, True):
            m = models.FCN32s(E2).load_synthetic(1337, device=dev).eval()
            ts = engine.TrainStep(m, emb, loss="mse", optimizer="adam", lr=1e-6, precision=torch.float32, bucket_mb=25, sharded=sharded)
            assert ts.world == 2
            # both ranks normalise by their own image's pixel count: the mean of the rank gradients is the two-image gradient
            ts.step(torch.from_numpy(x[rank:rank + 1]).to(dev), torch.from_numpy(t[rank:rank + 1]).to(dev))
            ts.gather_masters()
            torch.cuda.synchronize()
            if rank == 0:
                out["w%d" % sharded] = m.score_fr.weight.detach().cpu().numpy()
                if not sharded:
                    out["gw"] = (ts.flat_gw * 0.5).cpu().numpy()          # what the optimizer consumed: sum x 1/world
                    out["gb"] = (ts.flat_gb * 0.5).cpu().numpy()
        q.put(out)
        dist.barrier()
        dist.destroy_process_group()
    except Exception as ex:
        import traceback
        q.put({"rank": rank, "error": "%r\n%s" % (ex, traceback.format_exc())})


def test_two_ranks_mean_gradient():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 33700 + os.getpid() % 2000
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    for _ in procs:
        o = q.get(timeout=600)
        assert "error" not in o, o.get("error")
        res[o["rank"]] = o
    for p in procs:
        p.join(120)
    x, t = _dp_data()
    m = models.FCN32s(E2).load_synthetic(1337, device=torch.device("cuda", 0)).eval()
    ts = engine.TrainStep(m, _emb(K2, E2), loss="mse", optimizer="adam", lr=1e-6, precision=torch.float32)
    ts.step(cu(x), cu(t))
    torch.cuda.synchronize()
    gw, gb = ts.flat_gw.cpu().numpy(), ts.flat_gb.cpu().numpy()
    assert np.abs(res[0]["gw"] - gw).max() < 1e-5 * np.abs(gw).max()
    assert np.abs(res[0]["gb"] - gb).max() < 1e-5 * np.abs(gb).max()
    # replicated and sharded optimizer: the same updated weights
    assert np.array_equal(res[0]["w0"], res[0]["w1"])
