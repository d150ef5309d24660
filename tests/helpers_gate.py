"""A float64 numpy restatement of the soft seen/unseen gate in include/szn.h (szn_soft_gate_head), for the tests: the two experts'
log-sum-exps from helpers_seen_sweep.case_reference's similarities, the effective margin e = m32 - weight * (l_S - l_U), and
helpers_seen_sweep's predict / bins / crossing_histograms applied to e.  The cases are helpers_seen_sweep.CASES plus one with K = 2, one
class per group, where both log-sum-exps are exactly 0."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers_calib as HC  # noqa: E402
import helpers_msinfer as HM  # noqa: E402
import helpers_seen_sweep as HS  # noqa: E402

NEAR_TIE = HS.NEAR_TIE
K2 = "s32_e20_k2"                                   # the single-class-per-group case
NAMES = HS.NAMES                                    # the four cases the prediction tests run on
ALL_NAMES = NAMES + [K2]
N_TAUS = 9                                          # the unclear share of the issue's float64 check was taken with 9 taus


@functools.lru_cache(maxsize=None)
def case(name):
    """helpers_seen_sweep.case(name); K2: the map, seen-mask map and filters of "s32_e20_k21" with two of its class embeddings (classes 0
    and 1 of the new problem) and the labels folded to {0, 1} (the uncounted ones -1, -2, >= K kept).  Cached: treat as read-only."""
    if name != K2:
        return HS.case(name)
    c = dict(HS.case("s32_e20_k21"))
    t = c["target"]
    c["target"] = np.where((t >= 0) & (t < c["K"]), t % 2, t)
    c["emb"] = np.ascontiguousarray(c["emb"][[0, 5]])
    c["K"] = 2
    return c


def unseen_of(name, kind):
    """the unseen set of a case: helpers_seen_sweep.unseen_sets' four kinds; K2 has the two possible ones, "zero" = [0] and "high" = [1]"""
    c = case(name)
    if name == K2:
        return {"zero": [0], "high": [1]}[kind]
    return HS.unseen_sets(c["K"])[kind]


@functools.lru_cache(maxsize=None)
def sims(name):
    """-> (sim (B,H,W,K) float64, dead (B,H,W) bool: zero-norm pixels, every similarity NaN, m32: the kernel's float32 margin)"""
    if name != K2:
        r = HS.case_reference(name)
        return r["sim"], r["dead"], r["m32"]
    c = case(name)
    sim, _ = HM.view_sims(c["fmap"], c["S"], c["H"], c["W"], c["H"], c["W"], False, c["emb"])
    return sim, np.isnan(sim).all(axis=-1), HS.margin32(c["sm"], c["wt"], c["H"], c["W"])


def log_sum_exp(sim, members, best, temperature):
    """l_G = log sum_{k in members} exp((sim_k - best) / T) = -log P_G(argmax): in [0, log n_G]"""
    with np.errstate(invalid="ignore"):
        return np.log(np.exp((sim[..., np.asarray(members)] - best[..., None]) / temperature).sum(axis=-1))


def bound(weight, temperature, m):
    """|eff - e64| allowed: the project treats a cosine as known to NEAR_TIE; each of the four places a cosine enters D (the two bests,
    the two sums) carries 1 / T times that since log-sum-exp is 1-Lipschitz; 1e-5 for the fp32 expf / logf of numbers no larger than
    log K; 1e-6 |m| for the product and the sum with the margin"""
    w, t = float(np.float32(weight)), float(np.float32(temperature))
    return w * (4.0 / t * NEAR_TIE + 1e-5) + 1e-6 * np.abs(m)


@functools.lru_cache(maxsize=None)
def reference(name, kind, temperature, weight, n_taus=N_TAUS):
    """-> dict: A, Bc (the true in-group argmaxes, the first index winning; 0 on dead pixels), D, e64 (NaN on dead pixels), taus (n_taus
    ascending float32 values: e's own float32 values, one below, one above), bound (B,H,W), unclear (B,H,W) bool: a group's top-2 lead
    <= NEAR_TIE or e64 within the bound of any tau; dead pixels are clear (class 0); pred (G,B,H,W)"""
    c = case(name)
    sim, dead, m32 = sims(name)
    unseen = unseen_of(name, kind)
    seen = [k for k in range(c["K"]) if k not in set(unseen)]
    A, va, la = HC.group_best(sim, seen)
    Bc, vb, lb = HC.group_best(sim, unseen)
    t = float(np.float32(temperature))
    D = log_sum_exp(sim, seen, va, t) - log_sum_exp(sim, unseen, vb, t)
    m = m32.astype(np.float64)
    e64 = m - float(np.float32(weight)) * D
    assert np.array_equal(np.isnan(D), dead)
    A, Bc = np.where(dead, 0, A), np.where(dead, 0, Bc)
    taus = HS.taus_from(e64.astype(np.float32), n_taus)
    bd = bound(weight, temperature, m)
    with np.errstate(invalid="ignore"):
        near_tau = (np.abs(e64[None] - taus.astype(np.float64).reshape(-1, 1, 1, 1)) <= bd[None]).any(axis=0)
        unclear = ~dead & ((la <= NEAR_TIE) | (lb <= NEAR_TIE) | near_tau)
    return dict(A=A, Bc=Bc, la=la, lb=lb, D=D, e64=e64, taus=taus, bound=bd, unclear=unclear, dead=dead, n_seen=len(seen),
                n_unseen=len(unseen), pred=HS.predict(A, Bc, e64, taus))


def histograms(name, ref):
    """(G,K,K) for every tau of ref["taus"], directly from ref["pred"]"""
    c = case(name)
    return HS.histograms(c["target"], ref["pred"], c["K"])
