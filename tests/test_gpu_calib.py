"""GPU: the calibrated-stacking head (szn_calib_head, csrc/szn_fused_head.hip) through the C interface, on synthetic coarse maps (no
backbone), against szn_fused_head_strided, szn_confusion_hist_k and the float64 restatement in tests/helpers_calib.py.

Shapes: 33 x 47 pixels, B = 2 (a 2 x 2 map at stride 32, 14 x 14 at stride 8) and 70 x 90, B = 1 (3 x 3 and 18 x 18 maps: several cells with ragged
edges); (E, K) from (5, 21) to (300, 59) and K = 70 (class-set words above 64); 17 gammas from -0.5 to 0.5, 0.0 among them."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers_calib as HC  # noqa: E402
import helpers_msinfer as HM  # noqa: E402
from zeroshotsemanticsegmentation_amd import _lib as L  # noqa: E402

G0 = int(np.flatnonzero(HC.GAMMAS == 0.0)[0])


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _calib(c, gammas, pred_index=None, want_hist=True, coarse=None, target=None, hist=None):
    """szn_calib_head on case c -> (hist (G,K,K) numpy or None, pred numpy or None)"""
    lib = L.load()
    B, H, W, K, E, S = c["B"], c["H"], c["W"], c["K"], c["E"], c["S"]
    g = np.ascontiguousarray(gammas, dtype=np.float32)
    cm = _dev(c["coarse"] if coarse is None else coarse)
    emb = _dev(c["emb"])
    tgt = _dev(c["target"] if target is None else target) if want_hist else None
    if want_hist and hist is None:
        hist = torch.zeros(len(g), K, K, dtype=torch.int64, device="cuda")
    pred = torch.full((B, H, W), -7, dtype=torch.int64, device="cuda") if pred_index is not None else None
    nbytes = lib.szn_calib_head_workspace_bytes(S, B, c["h"], c["w"], E, K, len(g))
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    rc = lib.szn_calib_head(S, B, c["h"], c["w"], E, E, 0, H, W, HM.CROP[S], K, L.ptr(cm), L.ptr(emb), L.ptr(tgt),
                            L.class_set(c["unseen"]), len(g), g.ctypes.data_as(C.POINTER(C.c_float)), L.ptr(hist),
                            -1 if pred_index is None else pred_index, L.ptr(pred), L.ptr(ws), L.stream_ptr())
    assert rc == 0, lib.szn_last_error()
    torch.cuda.synchronize()
    return (hist.cpu().numpy() if want_hist else None), (pred.cpu().numpy() if pred is not None else None)


def _plain(c, coarse=None):
    """szn_fused_head_strided's pred"""
    lib = L.load()
    B, H, W, K, E, S = c["B"], c["H"], c["W"], c["K"], c["E"], c["S"]
    cm = _dev(c["coarse"] if coarse is None else coarse)
    emb = _dev(c["emb"])
    pred = torch.full((B, H, W), -7, dtype=torch.int64, device="cuda")
    ws = torch.empty(lib.szn_fused_head_workspace_bytes(B, c["h"], c["w"], E, K), dtype=torch.uint8, device="cuda")
    L.call("szn_fused_head_strided", S, B, c["h"], c["w"], E, E, 0, H, W, HM.CROP[S], K, L.ptr(cm), L.ptr(emb), None, None, None,
           L.ptr(pred), L.SZN_F32, None, L.ptr(ws), L.stream_ptr())
    torch.cuda.synchronize()
    return pred.cpu().numpy()


def _confusion(target, pred, K):
    hist = torch.zeros(3, K, K, dtype=torch.int64, device="cuda")
    lt, lp = _dev(target), _dev(pred)
    L.call("szn_confusion_hist_k", target.size, K, L.ptr(lt), L.ptr(lp), None, L.ptr(hist), L.stream_ptr())
    torch.cuda.synchronize()
    return hist[0].cpu().numpy()


@functools.lru_cache(maxsize=None)
def _sweep(name):
    """the 17-gamma call (hist, pred at gamma 0) and the 17 single-gamma predictions of the same head"""
    c = HC.case(name)
    hist, pred0 = _calib(c, c["gammas"], pred_index=G0)
    singles = [_calib(c, [g], pred_index=0, want_hist=False)[1] for g in c["gammas"]]
    return hist, pred0, singles


@pytest.mark.parametrize("name", HC.NAMES)
def test_gamma_zero_is_the_plain_head_bit_for_bit(name):
    c = HC.case(name)
    _, pred0, singles = _sweep(name)
    plain = _plain(c)
    assert plain.min() >= 0 and np.array_equal(pred0, plain) and np.array_equal(singles[G0], plain)
    # zero-norm pixels (every tap of their cell is zero): class 0 in both
    coarse = c["coarse"].copy()
    n = 1 if c["S"] == 32 else 5
    coarse[:, :n, :n] = 0.0
    sim, _ = HM.view_sims(coarse, c["S"], c["H"], c["W"], c["H"], c["W"], False, c["emb"])
    dead = np.isnan(sim).all(axis=-1)
    assert dead.any() and not dead.all()
    _, pz = _calib(c, c["gammas"], pred_index=G0, want_hist=False, coarse=coarse)
    plain_z = _plain(c, coarse)
    assert np.array_equal(pz, plain_z) and (pz[dead] == 0).all()
    for gi in (0, len(c["gammas"]) - 1):
        assert (_calib(c, c["gammas"], pred_index=gi, want_hist=False, coarse=coarse)[1][dead] == 0).all()


@pytest.mark.parametrize("name", HC.NAMES)
def test_histograms_are_the_exact_counts_of_the_single_gamma_predictions(name):
    c = HC.case(name)
    hist, _, singles = _sweep(name)
    for gi in range(len(c["gammas"])):
        assert np.array_equal(hist[gi], _confusion(c["target"], singles[gi], c["K"])), gi
    # the 17-gamma call returns the same prediction for pred_index = g
    for gi in (0, 3, G0 + 1, len(c["gammas"]) - 1):
        assert np.array_equal(_calib(c, c["gammas"], pred_index=gi, want_hist=False)[1], singles[gi]), gi
    n_unseen = [np.isin(p, c["unseen"]).sum() for p in singles]
    assert (np.diff(n_unseen) >= 0).all() and n_unseen[0] < n_unseen[-1]


@pytest.mark.parametrize("name", HC.NAMES)
def test_predictions_against_float64(name):
    c, ref = HC.case(name), HC.case_reference(name)
    _, _, singles = _sweep(name)
    got = np.stack(singles)
    share = ref["unclear"].any(axis=0).mean()
    print("%s: %.2f %% of the pixels unclear at some gamma, %.2f %% at most at one; %d of %d (gamma, pixel) decisions compared, %d differ"
          % (name, 100 * share, 100 * ref["unclear"].reshape(len(singles), -1).mean(axis=1).max(), (~ref["unclear"]).sum(), got.size,
             (got != ref["pred"])[~ref["unclear"]].sum()))
    assert share <= 0.05
    assert np.array_equal(got[~ref["unclear"]], ref["pred"][~ref["unclear"]])


def test_two_calls_are_bit_equal_and_hist_accumulates():
    c = HC.case("c2_s32_e300_k59")
    h1, p1 = _calib(c, c["gammas"], pred_index=5)
    assert L.last_kernel() == "calib_hist_kernel" and L.prev_kernel() == "calib_cell_kernel"
    h2, p2 = _calib(c, c["gammas"], pred_index=5)
    assert np.array_equal(h1, h2) and np.array_equal(p1, p2)
    acc = _dev(h1)
    h3, _ = _calib(c, c["gammas"], hist=acc)
    assert np.array_equal(h3, 2 * h1)
    _calib(c, c["gammas"], pred_index=5, want_hist=False)
    assert L.last_kernel() == "calib_cell_kernel"
    c8 = HC.case("c3_s8_e20_k33")
    _calib(c8, c8["gammas"])
    assert L.last_kernel() == "calib_hist_kernel" and L.prev_kernel() == "calib_cell_tab_kernel"
    _calib(c8, c8["gammas"], pred_index=0, want_hist=False)
    assert L.last_kernel() == "calib_cell_tab_kernel"


@pytest.mark.parametrize("name", ["c1_s32_e5_k21", "c3_s8_e20_k33"])
def test_labels_outside_the_classes_are_not_counted(name):
    c = HC.case(name)
    K = c["K"]
    hist, _, _ = _sweep(name)
    t = c["target"]
    assert (t == -1).any() and (t == -2).any()
    assert (hist.sum(axis=(1, 2)) == ((t >= 0) & (t < K)).sum()).all()
    t2 = t.copy()
    t2[:, 10:14, 7:30] = K
    t2[:, 20, :] = K + 200
    t2[:, 21, :] = np.iinfo(np.int64).min
    h2, _ = _calib(c, c["gammas"], target=t2)
    counted = (t2 >= 0) & (t2 < K)
    assert counted.sum() < ((t >= 0) & (t < K)).sum()
    assert (h2.sum(axis=(1, 2)) == counted.sum()).all()
    assert np.array_equal(h2.sum(axis=2)[0], np.bincount(t2[counted], minlength=K))


def test_launch_time_error_codes():
    lib = L.load()
    c = HC.case("c1_s32_e5_k21")
    cm, emb, tgt = _dev(c["coarse"]), _dev(c["emb"]), _dev(c["target"])
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    hist = torch.zeros(3, c["K"], c["K"], dtype=torch.int64, device="cuda")

    def head(gam=(-0.25, 0.0, 0.25), unseen=c["unseen"], hist=hist, target=tgt, stride=32):
        g = np.ascontiguousarray(gam, dtype=np.float32)
        return lib.szn_calib_head(stride, c["B"], c["h"], c["w"], c["E"], c["E"], 0, c["H"], c["W"], 19, c["K"], L.ptr(cm), L.ptr(emb),
                                  L.ptr(target), L.class_set(unseen), len(g), g.ctypes.data_as(C.POINTER(C.c_float)), L.ptr(hist), 0, None,
                                  L.ptr(ws), L.stream_ptr())
    assert head() == 0
    assert head(gam=(0.0, 0.0)) == -1 and head(gam=(0.0, float("nan"))) == -1
    assert head(unseen=[]) == -1 and head(unseen=list(range(c["K"]))) == -1 and head(unseen=[c["K"]]) == -1
    assert head(hist=None) == -1 and head(target=None) == -1 and head(stride=16) == -1
    torch.cuda.synchronize()
    assert hist.sum().item() == 3 * int(((c["target"] >= 0) & (c["target"] < c["K"])).sum())      # only the first call ran
