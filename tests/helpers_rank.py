"""helpers_rank.py -- numpy references of the hinge ranking loss (include/szn.h, szn_fused_rank_head).

  rank_ref            loss, d(score) and stats on a materialised (B,E,H,W) score, straight from the definition, in float64
  rank_coarse_ref     the direct float64 reference from a coarse NHWC map: upsample -> rank_ref -> the transposed upsample
  rank_cells_f32      a float32 restatement of the cosines the fused head's cell algebra derives (G, Q, w'G_k / |s| / n_k)
  rank_flip_pairs     the hinges within a width of their kink, and the step each adds to d(score) if a float32 evaluation flips it
  rank_flip_envelope  the sum of |step|: how far d(score) may move when float32 cosines land on the other side of a hinge
  CASES / inputs      the shapes and inputs of tests/test_gpu_rank_head.py part 1, built here so that the CPU suite can check them

Nothing here imports the package or the oracle (inputs() is handed the synth module by its caller).
"""
import os

import numpy as np

from helpers_simce import _bil, competing, labels, up_matrices

DELTA = 1e-4          # the near-kink width of rank_flip_envelope; float32 cosines stay within DELTA / 4 of the float64 ones


def _cosines(score, emb):
    s = np.asarray(score, np.float64).transpose(0, 2, 3, 1)                  # (B,H,W,E)
    e = np.asarray(emb, np.float64)
    n = np.linalg.norm(e, axis=1)
    n = np.where(n == 0, 1.0, n)
    sn = np.linalg.norm(s, axis=3, keepdims=True)                            # (B,H,W,1)
    return s, e, n, sn, (s @ e.T) / (sn * n)


def _pixels(target, K, exclude):
    comp = competing(K, exclude)
    in_range = (target >= 0) & (target < K)
    lbl = np.where(in_range, target, 0)
    counted = in_range & comp[lbl]
    negative = np.broadcast_to(comp, target.shape + (K,)).copy()
    np.put_along_axis(negative, lbl[..., None], False, axis=3)               # the label is no negative of its own pixel
    return comp, lbl, counted, negative


def rank_ref(score, target, emb, exclude, margin, hardest, want_grad=True):
    """score (B,E,H,W), target (B,H,W) int, emb (K,E) -> (loss, dscore (B,E,H,W) float64 or None, stats (B,2) float64)"""
    s, e, n, sn, cos = _cosines(score, emb)
    B, H, W, E = s.shape
    K = e.shape[0]
    comp, lbl, counted, negative = _pixels(target, K, exclude)
    cl = np.take_along_axis(cos, lbl[..., None], axis=3)
    v = np.where(negative, margin - cl + cos, -np.inf)                       # (B,H,W,K)
    if hardest:
        ks = v.argmax(axis=3)                                                # the lowest index on a tie
        vs = np.take_along_axis(v, ks[..., None], axis=3)[..., 0]
        term = np.maximum(vs, 0.0)
        c = np.zeros_like(cos)
        np.put_along_axis(c, ks[..., None], (vs > 0).astype(np.float64)[..., None], axis=3)
    else:
        term = np.maximum(v, 0.0).sum(axis=3)
        c = (v > 0).astype(np.float64)
    term = np.where(counted, term, 0.0)
    stats = np.stack([term.sum(axis=(1, 2)), counted.sum(axis=(1, 2)).astype(np.float64)], axis=1)
    loss = float(np.mean(stats[:, 0] / stats[:, 1]))
    if not want_grad:
        return loss, None, stats
    np.put_along_axis(c, lbl[..., None], -c.sum(axis=3, keepdims=True), axis=3)
    c = c * counted[..., None]
    # d term / d s = sum_k c_k (e_k / (|s| n_k) - cos_k s / |s|^2)
    g = (c / (sn * n)) @ e - (c * cos).sum(axis=3, keepdims=True) * s / sn ** 2
    g = g / (B * stats[:, 1])[:, None, None, None]
    return loss, np.ascontiguousarray(g.transpose(0, 3, 1, 2)), stats


def rank_coarse_ref(S, coarse, emb, target, exclude, margin, hardest, crop):
    """coarse (B,h,w,E) -> (loss, dcoarse (B,h,w,E) float64, stats)"""
    B, h, w, E = coarse.shape
    H, W = target.shape[1:]
    Uy, Ux = up_matrices(S, h, w, H, W, crop)
    score = np.einsum("yi,xj,bije->beyx", Uy, Ux, np.asarray(coarse, np.float64))
    loss, ds, stats = rank_ref(score, target, emb, exclude, margin, hardest)
    return loss, np.einsum("yi,xj,beyx->bije", Uy, Ux, ds), stats


def rank_cells_f32(S, coarse, emb, H, W, crop):
    """the cosines as the fused head derives them, in float32: per cell G[t][k] = C_t.e_k and Q[t][u] = C_t.C_u from the four tap
    vectors, per pixel |s|^2 = w'Qw and cos_k = (w'G_k) (1 / |s|) (1 / n_k).  coarse (B,h,w,E) -> cos (B,H,W,K) float32"""
    f = np.float32
    C = np.asarray(coarse, f)
    e = np.asarray(emb, f)
    B, h, w, E = C.shape
    n = np.sqrt((e * e).sum(axis=1, dtype=f)).astype(f)
    n = np.where(n == 0, f(1), n).astype(f)
    Cp = np.zeros((B, h + 2, w + 2, E), f)
    Cp[:, 1:h + 1, 1:w + 1] = C
    Tp = np.stack([Cp[:, a:a + h + 1, b:b + w + 1] for a in (0, 1) for b in (0, 1)], axis=3)        # (B,h+1,w+1,4,E)
    G = np.einsum("bijte,ke->bijtk", Tp, e).astype(f)
    Q = np.einsum("bijte,bijue->bijtu", Tp, Tp).astype(f)
    Y, X = np.arange(H) + crop, np.arange(W) + crop
    wy = np.stack([_bil(S, Y % S + S), _bil(S, Y % S)], 1)
    wx = np.stack([_bil(S, X % S + S), _bil(S, X % S)], 1)
    wt = (wy[:, None, :, None] * wx[None, :, None, :]).reshape(H, W, 4).astype(f)
    Gp = G[:, Y // S][:, :, X // S]                                          # (B,H,W,4,K)
    Qp = Q[:, Y // S][:, :, X // S]                                          # (B,H,W,4,4)
    ss = np.einsum("yxt,yxu,byxtu->byx", wt, wt, Qp).astype(f)
    rsn = (f(1) / np.sqrt(ss).astype(f)).astype(f)
    d = np.einsum("yxt,byxtk->byxk", wt, Gp).astype(f)
    return (d * (rsn[..., None] * (f(1) / n)).astype(f)).astype(f)


def rank_flip_pairs(score, target, emb, exclude, margin, hardest, delta=DELTA):
    """The loss is piecewise smooth in s: where a hinge sits within `delta` of its kink a float32 evaluation may take the other
    sub-gradient than the float64 reference.  Collects the reference's near-kink pairs -- |v_k| <= delta; for `hardest` of the best
    negative k* alone, and also every negative within delta of v_k* while v_k* > -delta (a float32 evaluation may crown it instead) --
    and for each the step its flip adds to d(score): (grad_s cos_k - grad_s cos_other) / (B N_b), other = the label, or k* for a
    near-tie.  score (B,E,H,W) -> (b, y, x) index arrays (m,) and the steps (m,E) float64, up to sign"""
    s, e, n, sn, cos = _cosines(score, emb)
    B, H, W, E = s.shape
    K = e.shape[0]
    comp, lbl, counted, negative = _pixels(target, K, exclude)
    cl = np.take_along_axis(cos, lbl[..., None], axis=3)
    v = np.where(negative & counted[..., None], margin - cl + cos, -np.inf)
    if hardest:
        ks = v.argmax(axis=3)
        vs = np.take_along_axis(v, ks[..., None], axis=3)[..., 0]
        b, y, x = np.nonzero(np.abs(vs) <= delta)
        k, o = ks[b, y, x], lbl[b, y, x]
        tie = (v >= (vs - delta)[..., None]) & (vs > -delta)[..., None] & np.isfinite(v)
        np.put_along_axis(tie, ks[..., None], False, axis=3)
        b2, y2, x2, k2 = np.nonzero(tie)
        b, y, x = np.concatenate([b, b2]), np.concatenate([y, y2]), np.concatenate([x, x2])
        k, o = np.concatenate([k, k2]), np.concatenate([o, ks[b2, y2, x2]])
    else:
        b, y, x, k = np.nonzero(np.abs(v) <= delta)
        o = lbl[b, y, x]
    nb = counted.sum(axis=(1, 2)).astype(np.float64)
    sp, snp = s[b, y, x], sn[b, y, x]                                        # (m,E), (m,1)
    gk = e[k] / (snp * n[k][:, None]) - cos[b, y, x, k][:, None] * sp / snp ** 2
    go = e[o] / (snp * n[o][:, None]) - cos[b, y, x, o][:, None] * sp / snp ** 2
    return (b, y, x), (gk - go) / (B * nb[b])[:, None]


def rank_flip_envelope(score, target, emb, exclude, margin, hardest, delta=DELTA):
    """the elementwise sum of |step| over rank_flip_pairs: how far d(score) may move when float32 hinges land on the other side of
    their kinks.  score (B,E,H,W) -> (envelope on d(score) (B,E,H,W) float64, >= 0; number of pairs)"""
    B, E, H, W = np.shape(score)
    (b, y, x), steps = rank_flip_pairs(score, target, emb, exclude, margin, hardest, delta)
    env = np.zeros((B, H, W, E))
    np.add.at(env, (b, y, x), np.abs(steps))
    return np.ascontiguousarray(env.transpose(0, 3, 1, 2)), len(b)


# ---- the inputs of tests/test_gpu_rank_head.py part 1 ------------------------------------------------------------------------------
CASES = [  # stride, B, H, W, E, K, c0, padding channels behind
    (32, 2, 70, 101, 20, 33, 0, 42),          # border cells with missing taps
    (32, 1, 1, 1, 20, 21, 0, 44),             # a one-pixel image
    (32, 1, 40, 50, 300, 59, 3, 1),           # a channel offset, E not a multiple of 64
    (8, 3, 33, 47, 20, 150, 0, 12),           # stride 8, KP > 64: three 64-class rounds of the dense-A tile, the last one partial
    (8, 2, 64, 64, 20, 256, 0, 0),            # KP = 256
]
# (map, margin, hardest): margin 2.5 exceeds every cos_label - cos_k, so no hinge has a kink within reach
VARIANTS = [("uniform", 0.1, 0), ("uniform", 0.1, 1), ("converged", 0.1, 0), ("converged", 0.1, 1), ("uniform", 2.5, 0)]
CROPS = {32: 19, 8: 31}


def embeddings(K, E, synth, golden):
    path = os.path.join(golden, "embeddings_context_%d.npy" % E)
    if os.path.exists(path):
        e = np.load(path).astype(np.float32)
        if e.shape[0] >= K:
            return np.ascontiguousarray(e[:K])
    return synth.make_embeddings(K, E, seed=5)


def inputs(case, kind, synth, golden):
    """-> dict(emb (K,E) f32, exclude, target (B,H,W) int64, coarse (B,h,w,E) f32 -- the embedding channels alone --, h, w, crop, seed)"""
    S, B, H, W, E, K, c0, extra = case
    crop = CROPS[S]
    h, w = (H + crop + S - 1) // S, (W + crop + S - 1) // S
    seed = S * 1000 + E + K
    emb = embeddings(K, E, synth, golden)
    exclude = list(range(0, K, 3))                  # every third class does not compete
    target = labels(B, H, W, K, exclude, seed + 1)
    if kind == "uniform":
        coarse = synth.uniform(seed, (B, h, w, E), -2, 2)
    else:                                           # near-converged: every position sits at its label's embedding, 1 % noise
        yy = np.clip(S * np.arange(h) + S // 2 - crop, 0, H - 1)
        xx = np.clip(S * np.arange(w) + S // 2 - crop, 0, W - 1)
        lab = target[:, yy][:, :, xx]
        lab = np.where((lab < 0) | (lab >= K), 0, lab)
        base = emb[lab]
        nrm = np.linalg.norm(base, axis=-1, keepdims=True)
        noise = np.random.RandomState(seed + 7).randn(B, h, w, E).astype(np.float32)
        coarse = (base + np.float32(1e-2) * nrm * noise).astype(np.float32)
    return dict(emb=emb, exclude=exclude, target=target, coarse=coarse, h=h, w=w, crop=crop, seed=seed)
