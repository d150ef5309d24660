"""helpers_bias.py -- numpy reference of sim_ce with the unseen-bias term on hidden pixels (include/szn.h, szn_fused_simce_bias_head).

  bias_ref      loss, d(score) and stats on a materialised (B,E,H,W) score, straight from the definition, in float64
  unseen_prob   P_U = sum_{u in U} softmax_u(cos / T) over all classes per pixel, in float64 (what the term pushes up)
  hide          marks a share of a target's pixels hidden
  unseen_of     the unseen set the GPU tests pair with helpers_rank.inputs' exclude set
  inputs        helpers_rank.inputs with hidden pixels; its near-converged map puts every hidden position at a SEEN class's embedding

Nothing here imports the package or the oracle (inputs() is handed the synth module by its caller).
"""
import numpy as np

import helpers_rank as R
from helpers_simce import competing, labels  # noqa: F401  (labels: re-exported for the tests' own targets)

HIDDEN = -3           # datasets.HIDDEN_LABEL (tests/test_bias_ref.py checks the two agree)


def _lse(z, mask):
    """log sum_{k in mask} exp(z_k) over the last axis with the masked maximum subtracted, and the shifted exponentials (0 outside)"""
    zm = np.where(mask, z, -np.inf)
    m = zm.max(axis=-1, keepdims=True)
    ex = np.exp(zm - m)
    return m[..., 0] + np.log(ex.sum(axis=-1)), ex / ex.sum(axis=-1, keepdims=True)


def _cos(score, emb):
    s = np.asarray(score, np.float64).transpose(0, 2, 3, 1)                  # (B,H,W,E)
    e = np.asarray(emb, np.float64)
    n = np.linalg.norm(e, axis=1)
    n = np.where(n == 0, 1.0, n)
    sn = np.linalg.norm(s, axis=3, keepdims=True)                            # (B,H,W,1)
    return s, e, n, sn, (s @ e.T) / (sn * n)


def bias_ref(score, target, emb, exclude, T, unseen, weight, hidden=HIDDEN, want_grad=True):
    """score (B,E,H,W), target (B,H,W) int, emb (K,E) -> (loss, dscore (B,E,H,W) float64 or None, stats (B,2) float64).
    labelled pixel (0 <= label < K, not in exclude): logsumexp_{k not in exclude} z_k - z_label; hidden pixel (label == hidden):
    weight (logsumexp_{all k} z_k - logsumexp_{u in unseen} z_u); stats[b] = {sum of terms, labelled + hidden}"""
    s, e, n, sn, cos = _cos(score, emb)
    B, H, W, E = s.shape
    K = e.shape[0]
    comp = competing(K, exclude)
    in_u = ~competing(K, unseen)
    assert in_u.any() and not in_u.all() and hidden < -1 and weight > 0
    z = cos / T
    in_range = (target >= 0) & (target < K)
    lbl = np.where(in_range, target, 0)
    labelled = in_range & comp[lbl]
    hid = target == hidden
    lse_s, p_s = _lse(z, comp)                                               # over the competing classes
    lse_a, p_a = _lse(z, np.ones(K, bool))                                   # over all classes
    lse_u, q = _lse(z, in_u)                                                 # over the unseen set: q_k = p_k / P_U, formed without P_U
    zl = np.take_along_axis(z, lbl[..., None], axis=3)[..., 0]
    term = np.where(labelled, lse_s - zl, np.where(hid, weight * (lse_a - lse_u), 0.0))
    stats = np.stack([term.sum(axis=(1, 2)), (labelled | hid).sum(axis=(1, 2)).astype(np.float64)], axis=1)
    loss = float(np.mean(stats[:, 0] / stats[:, 1]))
    if not want_grad:
        return loss, None, stats
    y = np.zeros_like(p_s)
    np.put_along_axis(y, lbl[..., None], 1.0, axis=3)
    c = ((p_s - y) * labelled[..., None] + weight * (p_a - q) * hid[..., None]) / T          # (B,H,W,K)
    # d term / d s = sum_k c_k (e_k / (|s| n_k) - cos_k s / |s|^2)
    g = (c / (sn * n)) @ e - (c * cos).sum(axis=3, keepdims=True) * s / sn ** 2
    g = g / (B * stats[:, 1])[:, None, None, None]
    return loss, np.ascontiguousarray(g.transpose(0, 3, 1, 2)), stats


def unseen_prob(score, emb, T, unseen):
    """P_U per pixel (B,H,W), float64"""
    _, e, _, _, cos = _cos(score, emb)
    z = cos / T
    p = np.exp(z - z.max(axis=3, keepdims=True))
    p /= p.sum(axis=3, keepdims=True)
    return p[..., ~competing(e.shape[0], unseen)].sum(axis=3)


def hide(target, share, seed, hidden=HIDDEN):
    """a copy of `target` with about `share` of its pixels (whatever they held) marked hidden; a one-pixel target: that pixel"""
    t = np.array(target, dtype=np.int64, copy=True)
    if t[0].size == 1:
        t[:] = hidden
    else:
        t[np.random.RandomState(seed).rand(*t.shape) < share] = hidden
    return t


def unseen_of(exclude, K):
    """the unseen set paired with an exclude set in the GPU tests: the exclude set without its first class, plus the first class
    outside it -- so one class is excluded but seen, and one is unseen but competes: the head must keep the two sets apart"""
    extra = next(k for k in range(K) if k not in exclude)
    return sorted(set(exclude[1:]) | {extra})


def inputs(case, kind, synth, golden, share=0.2):
    """helpers_rank.inputs(case, kind) with `share` of the pixels hidden and unseen = unseen_of(exclude); "converged": the positions
    whose own pixel is hidden or carries an unseen class sit at the embedding of a class OUTSIDE unseen instead (1 % noise), so every
    position of the map is at a seen class and P_U is small at the hidden pixels"""
    S, B, H, W, E, K = case[:6]
    I = dict(R.inputs(case, "uniform" if kind == "uniform" else "converged", synth, golden))
    I["unseen"] = unseen_of(I["exclude"], K)
    I["target"] = hide(I["target"], share, I["seed"] + 11)
    if kind != "uniform":
        crop, h, w, emb = I["crop"], I["h"], I["w"], I["emb"]
        yy = np.clip(S * np.arange(h) + S // 2 - crop, 0, H - 1)
        xx = np.clip(S * np.arange(w) + S // 2 - crop, 0, W - 1)
        lab = I["target"][:, yy][:, :, xx]
        seen = np.array([k for k in range(K) if k not in I["unseen"]])
        pick = seen[np.random.RandomState(I["seed"] + 13).randint(0, len(seen), size=lab.shape)]
        base = emb[pick]
        nrm = np.linalg.norm(base, axis=-1, keepdims=True)
        noise = np.random.RandomState(I["seed"] + 7).randn(B, h, w, E).astype(np.float32)
        move = (lab == HIDDEN) | np.isin(lab, I["unseen"])
        I["coarse"] = np.where(move[..., None], (base + np.float32(1e-2) * nrm * noise).astype(np.float32), I["coarse"])
    return I
