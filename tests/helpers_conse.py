"""A numpy float64 restatement of the ConSE contract in include/szn.h (szn_conse_head), for the tests, built from the pieces of
tests/helpers_msinfer.py (up_crop, first_argmax) and tests/helpers_calib.py (group_best, predict, histograms, the geometry).  Also
the synthetic cases the CPU and the GPU tests share, and the two error bounds that decide which pixels fp32 may legitimately
assign otherwise.

The bounds (u = 2^-24, the unit roundoff of fp32; first order in u), from the kernel's rounding count:

  logits.  z is a chain of four fmaf over the taps: four roundings of partial sums no larger than the same blend of the absolute values,
      zeta = max_k sum_t w_t |C_t[k]| of the pixel.  So |z_fp32 - z| <= 4 u zeta, and two logits can change order only when they are
      closer than
          GAP = 8 u zeta.
      The float64 gap between the T-th and the (T+1)-th seen logit must exceed it, or S itself is in doubt.

  similarities.  With n = |S|, A = sum_t p_t |e_t| and kappa = A / |f| (>= 1: how much the mixture cancels):
      exponent:   p does not depend on the value that is subtracted from every logit, so the error of the maximum does not count; z_t's
                  own error 4 u zeta and the rounding of a difference below 2 zeta remain: 6 u zeta absolute;
      e_t:        relative error 6 u zeta + 2 u (expf within 1 ulp);
      p_t:        e_t / sum e: the sum's relative error is at most its terms' plus n - 1 additions, then one division:
                      eps_p = (12 zeta + n + 4) u   relative, per entry.
                  The kernel's f . e_k and |f|^2 are those of ONE perturbed mixture f~ = sum_t p~_t e_t, |f~ - f| <= eps_p A, plus their
                  own roundings.  A cosine moves by at most the angle its vector turns: |cos(f~, e_k) - cos(f, e_k)| <= eps_p A / |f| =
                  eps_p kappa;
      f . e_k:    G rounded once and the n-term fmaf chain: (n + 1) u relative to sum_t p_t |e_t| |e_k| = A |e_k|, i.e. (n + 1) u kappa
                  on the cosine;
      |f|:        |f|^2 the same with two factors: (2 n + 2) u A^2 absolute; the root halves the relative error and rounds once:
                  (n + 1) u kappa^2 + u relative;
      en[k]:      sqrt of a rounded value: 1.5 u; the product |f| en[k] and the division: 2 u.
      sim[k] = (f . e_k) / (|f| en[k]) with |sim| <= 1:
          |sim_fp32 - sim| <= BOUND = (12 zeta + n + 4) kappa u + (n + 1) (kappa + kappa^2) u + 5 u.
      A difference of two similarities (the lead inside a group, the margin m = va - vb) is off by at most 2 BOUND + 2 u.

A pixel is unclear at gamma g when the gap is <= GAP, when the lead of a or of b inside its group is <= 2 BOUND + 2 u (a or b itself is
then in doubt), or when |m - gamma_g| <= 2 BOUND + 2 u.  A vanishing |f| makes kappa, and with it BOUND, unbounded: such a pixel is
unclear."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers_calib as HC  # noqa: E402
import helpers_msinfer as HM  # noqa: E402

U = HM.U
GAMMAS = np.linspace(-0.5, 0.5, 17).astype(np.float32)          # contains 0.0 exactly
assert GAMMAS[8] == 0.0
UNCLEAR_CAP = 0.01

#        name: (stride, E, K, T, H, W, B, seed)
CASES = {
    "c1_s32_e5_k21_t1": (32, 5, 21, 1, 33, 47, 2, 201),
    "c2_s8_e5_k21_t5": (8, 5, 21, 5, 33, 47, 2, 202),
    "c3_s32_e300_k59_t10": (32, 300, 59, 10, 33, 47, 2, 203),
    "c4_s8_e20_k33_t5": (8, 20, 33, 5, 70, 90, 1, 204),
    "c5_s32_e20_k70_t16": (32, 20, 70, 16, 70, 90, 1, 205),
    "c6_s8_e300_k59_t3": (8, 300, 59, 3, 33, 47, 2, 206),
    "c7_s8_e5_k21_t16_all_seen": (8, 5, 21, 16, 33, 47, 2, 207),          # T >= n_seen = 14
    "c8_s32_e20_k130_t10_global": (32, 20, 130, 10, 33, 47, 2, 208),       # G outside LDS
    "c9_s8_e20_k130_t8_global": (8, 20, 130, 8, 70, 90, 1, 209),
}
NAMES = sorted(CASES)
# include/szn.h: G is copied into LDS when taps (4 K per cell; 1 cell per block at stride 32, 4 at stride 8) + en (K) + G (K (K | 1))
# floats fit 64 KiB: K <= 119 at stride 8, K <= 125 at stride 32
GLOBAL_G = {n for n in NAMES if 4 * ((4 if CASES[n][0] == 32 else 16) * CASES[n][2] + CASES[n][2] + CASES[n][2] * (CASES[n][2] | 1)) > 65536}
assert GLOBAL_G == {n for n in NAMES if CASES[n][2] == 130}


def embeddings(E, K):
    """K rows of width E: helpers_calib's up to the 177 it has (no two rows parallel inside a group), beyond that rows of a seeded
    generator"""
    rows = np.load(os.path.join(HM.GOLDEN, "embeddings_context_%d.npy" % E)).astype(np.float32)
    have = min(K, 3 * rows.shape[0])
    emb = HC.embeddings(E, have)
    if K > have:
        emb = np.concatenate([emb, np.random.RandomState(7).randn(K - have, E).astype(np.float32)], axis=0)
    return np.ascontiguousarray(emb)


@functools.lru_cache(maxsize=None)
def case(name):
    """a synthetic case: a logit map 3 N(0,1) on the h x w map the backbone gives for H x W; labels with -1 / -2 regions.  Cached: treat
    as read-only."""
    S, E, K, T, H, W, B, seed = CASES[name]
    rng = np.random.RandomState(seed)
    h, w = HM.coarse_size(H, S), HM.coarse_size(W, S)
    coarse = (3.0 * rng.randn(B, h, w, K)).astype(np.float32)
    target = rng.randint(0, K, (B, H, W)).astype(np.int64)
    target[:, :3, :5] = -1
    target[:, -2:, :] = -2
    return dict(S=S, E=E, K=K, T=T, B=B, H=H, W=W, h=h, w=w, coarse=coarse, emb=embeddings(E, K), target=target,
                unseen=list(range(2, K, 3)), gammas=GAMMAS)


def forced(a, b, m, target, unseen):
    """the -fu rule: b where the target names an unseen class, a elsewhere; 0 where m is NaN"""
    out = np.where(np.isin(target, list(unseen)), b, a)
    return np.where(np.isnan(m), 0, out).astype(np.int64)


def reference(S, H, W, coarse, emb, unseen, top_t, gammas):
    """-> dict: z (B,H,W,K) float64, top (B,H,W,n) the classes of S in order, p, sim (B,H,W,K), a, b, m, pred (G,B,H,W), gap, kappa,
    bound, unclear (G,B,H,W) bool (the module docstring)"""
    e = np.asarray(emb, dtype=np.float64)
    K = e.shape[0]
    is_unseen = np.zeros(K, dtype=bool)
    is_unseen[list(unseen)] = True
    seen = np.flatnonzero(~is_unseen)
    z = HM.up_crop(coarse, S, H, W, HM.CROP[S])
    zs = z[..., seen]
    order = np.argsort(-zs, axis=-1, kind="stable")                   # (z descending, class index ascending)
    zsort = np.take_along_axis(zs, order, axis=-1)
    n = min(int(top_t), len(seen))
    gap = zsort[..., n - 1] - zsort[..., n] if n < len(seen) else np.full(zs.shape[:-1], np.inf)
    top = seen[order[..., :n]]
    ex = np.exp(zsort[..., :n] - zsort[..., :1])
    p = ex / ex.sum(axis=-1, keepdims=True)
    f = (p[..., None] * e[top]).sum(axis=-2)                          # (B,H,W,E)
    en = np.linalg.norm(e, axis=1)
    fnorm = np.linalg.norm(f, axis=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        sim = (f @ e.T) / (np.where(fnorm == 0, 1.0, fnorm)[..., None] * np.where(en == 0, 1.0, en))
        kappa = (p * en[top]).sum(axis=-1) / fnorm
    a, va, lead_a = HC.group_best(sim, seen)
    b, vb, lead_b = HC.group_best(sim, np.flatnonzero(is_unseen))
    m = va - vb
    zeta = HM.up_crop(np.abs(np.asarray(coarse, dtype=np.float64)), S, H, W, HM.CROP[S]).max(axis=-1)
    gap_bound = 8.0 * U * zeta
    bound = ((12.0 * zeta + n + 4) * kappa + (n + 1) * (kappa + kappa ** 2) + 5.0) * U
    diff = 2.0 * bound + 2.0 * U
    g = np.asarray(gammas, dtype=np.float64).reshape(-1, 1, 1, 1)
    with np.errstate(invalid="ignore"):
        shaky = ~(gap > gap_bound) | ~((lead_a > diff) & (lead_b > diff))
        unclear = shaky[None] | ~(np.abs(m[None] - g) > diff[None])
    return dict(z=z, top=top, p=p, sim=sim, a=a, b=b, m=m, pred=HC.predict(a, b, m, gammas), gap=gap, gap_bound=gap_bound, kappa=kappa,
                bound=bound, shaky=shaky, unclear=unclear)


@functools.lru_cache(maxsize=None)
def case_reference(name):
    c = case(name)
    return reference(c["S"], c["H"], c["W"], c["coarse"], c["emb"], c["unseen"], c["T"], c["gammas"])


def unclear_share(ref):
    """the largest share of unclear pixels over the gammas"""
    return float(ref["unclear"].reshape(ref["unclear"].shape[0], -1).mean(axis=1).max())
