"""helpers_simce.py -- numpy references of the similarity cross-entropy loss (include/szn.h, szn_fused_simce_head).

  simce_ref        loss, d(score) and stats on a materialised (B,E,H,W) score, straight from the definition, in float64
  up_matrices      the bilinear deconv + crop of stride S as two float64 matrices (rows: output pixels, columns: coarse positions)
  simce_coarse_ref the direct float64 reference from a coarse NHWC map: upsample -> simce_ref -> the transposed upsample
  simce_cells_f32  a float32 restatement of the per-cell algebra the fused head runs (G, Q, per-pixel softmax, A, Bm, gather)

Nothing here imports the package or the oracle.
"""
import numpy as np


def competing(K, exclude):
    m = np.ones(K, dtype=bool)
    for k in exclude or []:
        m[int(k)] = False
    return m


def simce_ref(score, target, emb, exclude, T, want_grad=True):
    """score (B,E,H,W), target (B,H,W) int, emb (K,E) -> (loss, dscore (B,E,H,W) float64 or None, stats (B,2) float64)"""
    s = np.asarray(score, np.float64).transpose(0, 2, 3, 1)                  # (B,H,W,E)
    e = np.asarray(emb, np.float64)
    B, H, W, E = s.shape
    K = e.shape[0]
    comp = competing(K, exclude)
    n = np.linalg.norm(e, axis=1)
    n = np.where(n == 0, 1.0, n)
    sn = np.linalg.norm(s, axis=3, keepdims=True)                            # (B,H,W,1)
    cos = (s @ e.T) / (sn * n)                                               # (B,H,W,K)
    z = np.where(comp, cos / T, -np.inf)
    m = z.max(axis=3, keepdims=True)
    ex = np.exp(z - m)
    lse = m[..., 0] + np.log(ex.sum(axis=3))
    in_range = (target >= 0) & (target < K)
    lbl = np.where(in_range, target, 0)
    counted = in_range & comp[lbl]
    zl = np.take_along_axis(cos / T, lbl[..., None], axis=3)[..., 0]
    term = np.where(counted, lse - zl, 0.0)
    stats = np.stack([term.sum(axis=(1, 2)), counted.sum(axis=(1, 2)).astype(np.float64)], axis=1)
    loss = float(np.mean(stats[:, 0] / stats[:, 1]))
    if not want_grad:
        return loss, None, stats
    p = ex / ex.sum(axis=3, keepdims=True)                                   # 0 outside the competing set
    y = np.zeros_like(p)
    np.put_along_axis(y, lbl[..., None], 1.0, axis=3)
    c = (p - y) * counted[..., None] / T                                     # (B,H,W,K)
    # d term / d s = sum_k c_k (e_k / (|s| n_k) - cos_k s / |s|^2)
    g = (c / (sn * n)) @ e - (c * cos).sum(axis=3, keepdims=True) * s / sn ** 2
    g = g / (B * stats[:, 1])[:, None, None, None]
    return loss, np.ascontiguousarray(g.transpose(0, 3, 1, 2)), stats


def _bil(S, t):
    return 1.0 - np.abs(t - (S - 0.5)) / S


def up_matrices(S, h, w, H, W, crop):
    """Uy (H,h), Ux (W,w): score[y, x] = sum_ij Uy[y, i] Ux[x, j] coarse[i, j] (ConvTranspose2d(2 S, stride S) + crop)"""
    def one(n_out, n_in):
        U = np.zeros((n_out, n_in))
        for o in range(n_out):
            Y = o + crop
            I, t = Y // S, Y % S
            if 0 <= I - 1 < n_in:
                U[o, I - 1] = _bil(S, t + S)
            if I < n_in:
                U[o, I] = _bil(S, t)
        return U
    return one(H, h), one(W, w)


def simce_coarse_ref(S, coarse, emb, target, exclude, T, crop):
    """coarse (B,h,w,E) -> (loss, dcoarse (B,h,w,E) float64, stats)"""
    B, h, w, E = coarse.shape
    H, W = target.shape[1:]
    Uy, Ux = up_matrices(S, h, w, H, W, crop)
    score = np.einsum("yi,xj,bije->beyx", Uy, Ux, np.asarray(coarse, np.float64))
    loss, ds, stats = simce_ref(score, target, emb, exclude, T)
    return loss, np.einsum("yi,xj,beyx->bije", Uy, Ux, ds), stats


def simce_cells_f32(S, coarse, emb, target, exclude, T, crop):
    """the fused head's algebra in float32: per cell G[t][k] = C_t.e_k and Q[t][u] = C_t.C_u from the four tap vectors, per pixel
    |s|^2 = w'Qw, cos_k = w'G_k / (|s| n_k), the softmax over the competing classes, A[t][k] += w_t (y_k - p_k) / (T |s| n_k),
    Bm[t][u] += w_t w_u (cos_label - sum_k p_k cos_k) / (T |s|^2), then dC_t = (sum_u Bm[t][u] C_u - sum_k A[t][k] e_k) / (B N_b)
    summed over the cells a position is a tap of.  -> (loss, dcoarse (B,h,w,E) float32, stats)"""
    f = np.float32
    C = np.asarray(coarse, f)
    e = np.asarray(emb, f)
    B, h, w, E = C.shape
    H, W = target.shape[1:]
    K = e.shape[0]
    comp = competing(K, exclude)
    n = np.sqrt((e * e).sum(axis=1, dtype=f)).astype(f)
    n = np.where(n == 0, f(1), n).astype(f)
    Cp = np.zeros((B, h + 2, w + 2, E), f)
    Cp[:, 1:h + 1, 1:w + 1] = C
    # taps of cell (I, J), I in [0, h], J in [0, w]: t = 2 a + b -> position (I - 1 + a, J - 1 + b)
    Tp = np.stack([Cp[:, a:a + h + 1, b:b + w + 1] for a in (0, 1) for b in (0, 1)], axis=3)        # (B,h+1,w+1,4,E)
    G = np.einsum("bijte,ke->bijtk", Tp, e).astype(f)
    Q = np.einsum("bijte,bijue->bijtu", Tp, Tp).astype(f)
    Y, X = np.arange(H) + crop, np.arange(W) + crop
    wy = np.stack([_bil(S, Y % S + S), _bil(S, Y % S)], 1)
    wx = np.stack([_bil(S, X % S + S), _bil(S, X % S)], 1)
    wt = (wy[:, None, :, None] * wx[None, :, None, :]).reshape(H, W, 4).astype(f)
    b, y, x = np.meshgrid(np.arange(B), np.arange(H), np.arange(W), indexing="ij")
    b, y, x = b.ravel(), y.ravel(), x.ravel()
    ci, cj = Y[y] // S, X[x] // S
    wp = wt[y, x]                                                            # (n,4)
    Gp, Qp = G[b, ci, cj], Q[b, ci, cj]                                      # (n,4,K), (n,4,4)
    ss = np.einsum("nt,nu,ntu->n", wp, wp, Qp).astype(f)
    sn = np.sqrt(ss).astype(f)
    cos = (np.einsum("nt,ntk->nk", wp, Gp).astype(f) / (sn[:, None] * n[None, :])).astype(f)
    t = target[b, y, x]
    in_range = (t >= 0) & (t < K)
    lbl = np.where(in_range, t, 0)
    counted = in_range & comp[lbl]
    inv_t = f(1) / f(T)
    z = np.where(comp, cos * inv_t, f(-np.inf)).astype(f)
    m = z.max(axis=1)
    ex = np.exp((z - m[:, None]).astype(f)).astype(f)
    sm = ex.sum(axis=1, dtype=f)
    cl = cos[np.arange(len(t)), lbl]
    term = ((m - cl * inv_t) + np.log(sm).astype(f)).astype(f)
    stats = np.zeros((B, 2))
    np.add.at(stats[:, 0], b[counted], term[counted].astype(np.float64))
    np.add.at(stats[:, 1], b[counted], 1.0)
    loss = float(np.mean(stats[:, 0] / stats[:, 1]))
    p = (ex / sm[:, None]).astype(f)
    yk = np.zeros_like(p)
    yk[np.arange(len(t)), lbl] = 1
    coef = ((yk - p) * (inv_t / sn)[:, None] / n[None, :]).astype(f) * counted[:, None]
    bco = ((cl - (p * cos).sum(axis=1, dtype=f)) * inv_t / ss).astype(f) * counted
    A = np.zeros((B, h + 1, w + 1, 4, K), f)
    Bm = np.zeros((B, h + 1, w + 1, 4, 4), f)
    np.add.at(A, (b, ci, cj), (wp[:, :, None] * coef[:, None, :]).astype(f))
    np.add.at(Bm, (b, ci, cj), (wp[:, :, None] * wp[:, None, :] * bco[:, None, None]).astype(f))
    dT = (np.einsum("bijtu,bijue->bijte", Bm, Tp).astype(f) - np.einsum("bijtk,ke->bijte", A, e).astype(f)).astype(f)
    dCp = np.zeros_like(Cp)
    for tt, (a, bb) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)]):
        dCp[:, a:a + h + 1, bb:bb + w + 1] += dT[:, :, :, tt]
    scale = (f(1) / (f(B) * stats[:, 1].astype(f))).astype(f)
    return loss, (dCp[:, 1:h + 1, 1:w + 1] * scale[:, None, None, None]).astype(f), stats


def labels(B, H, W, K, exclude, seed, block=8):
    """block-constant labels over all K classes (so some are excluded ones) with -1, -2 and K + 1 sprinkled in"""
    rs = np.random.RandomState(seed)
    hb, wb = (H + block - 1) // block, (W + block - 1) // block
    t = rs.randint(0, K, size=(B, hb, wb)).repeat(block, axis=1).repeat(block, axis=2)[:, :H, :W].astype(np.int64)
    if H * W > 1:
        r = rs.rand(B, H, W)
        t[r < 0.04] = -1
        t[(r >= 0.04) & (r < 0.07)] = -2
        t[(r >= 0.07) & (r < 0.09)] = K + 1
        if exclude:
            t[(r >= 0.09) & (r < 0.11)] = exclude[0]
    comp = competing(K, exclude)
    for i in range(B):              # every image keeps at least one counted pixel
        ok = (t[i] >= 0) & (t[i] < K)
        if not (ok & comp[np.where(ok, t[i], 0)]).any():
            t[i, 0, 0] = int(np.nonzero(comp)[0][0])
    return t
