"""GPU: class-prototype pooling (szn_class_proto, csrc/szn_proto.hip) through the C interface, on the synthetic coarse maps of
tests/helpers_calib.py, both modes: (a) counts exact, sums within the derived bounds of the float64 restatement (RAW: n_add 2^-52 A
against the exact table form; UNIT: the per-pixel similarity bound summed over the pixels, plus the RAW term); (b) a class set
restricts, accumulation is one exact add, two calls are bit-equal; (c) padded maps (ldc > E, c0 > 0, NaN in the padding) give the
compact map's bits; (d) single-pixel classes at the corners and on a cell border; (e) an all-zero region is counted and not summed, no
NaN; (f) labels -1 / -2 / -3 / >= K leave everything untouched.

Shapes: helpers_calib.CASES (strides 32 / 8, E 5-300, K 21-70, 33 x 47 at B = 2, 70 x 90 at B = 1)."""
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
import helpers_proto as HP  # noqa: E402
from zeroshotsemanticsegmentation_amd import _lib as L  # noqa: E402

MODES = {"raw": L.PROTO_RAW, "unit": L.PROTO_UNIT}
SENTINEL = -7


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()           # a copy: the cached cases are read-only


def _proto(c, labels, mode, classes=None, into=None, coarse=None, ldc=None, c0=0):
    """szn_class_proto on case c (or on another map of its geometry) -> (sums (K,E) float64, counts (K,2) int64) numpy.  into = (sums,
    counts) numpy: the call accumulates into copies of them.  coarse with ldc / c0: a padded map (B,h,w,ldc)."""
    lib = L.load()
    coarse = c["coarse"] if coarse is None else coarse
    S, E, K, H, W = c["S"], c["E"], c["K"], labels.shape[1], labels.shape[2]
    B, h, w = coarse.shape[:3]
    ldc = coarse.shape[3] if ldc is None else ldc
    cm, lb = _dev(coarse), _dev(labels)
    if into is None:
        sums = torch.full((K, E), float(SENTINEL), dtype=torch.float64, device="cuda")
        counts = torch.full((K, 2), SENTINEL, dtype=torch.int64, device="cuda")
    else:
        sums, counts = _dev(into[0]), _dev(into[1])
    nbytes = lib.szn_class_proto_workspace_bytes(S, B, h, w, E, K)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    rc = lib.szn_class_proto(S, B, h, w, E, ldc, c0, H, W, HM.CROP[S], K, L.ptr(cm), L.ptr(lb), None if classes is None else L.class_set(classes),
                             MODES[mode], int(into is not None), L.ptr(sums), L.ptr(counts), L.ptr(ws), L.stream_ptr())
    assert rc == 0, lib.szn_last_error()
    torch.cuda.synchronize()
    assert L.last_kernel() == "proto_finalize_kernel" and L.prev_kernel() == "proto_reduce_kernel"
    return sums.cpu().numpy(), counts.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _run(name, mode):
    c = HC.case(name)
    return _proto(c, c["target"], mode)


def _reference(c, coarse, labels, mode):
    """helpers_proto.reference; the RAW sums come from the exact table form, which is what raw_bound is derived against"""
    ref = HP.reference(c["S"], c["H"], c["W"], coarse, labels, c["K"], None, mode)
    if mode == "raw":
        ref["sums"] = HP.raw_reference_exact(c["S"], c["H"], c["W"], coarse, labels, c["K"])[0]
    return ref


@functools.lru_cache(maxsize=None)
def _ref(name, mode):
    c = HC.case(name)
    return _reference(c, c["coarse"], c["target"], mode)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("mode", ["raw", "unit"])
@pytest.mark.parametrize("name", HC.NAMES)
def test_sums_and_counts_against_float64(name, mode):
    """(a) counts exact; sums within the bound of the mode"""
    c, (sums, counts), ref = HC.case(name), _run(name, mode), _ref(name, mode)
    npos = c["B"] * c["h"] * c["w"]
    assert np.array_equal(counts, ref["counts"])
    bound = HP.raw_bound(ref, npos) if mode == "raw" else HP.unit_bound(ref, npos)
    err = np.abs(sums - ref["sums"])
    i = np.unravel_index(np.argmax(err - bound), err.shape)
    print("%s %s: max |sums - ref| %.3e (bound there %.3e); worst err / bound %.3g at k=%d e=%d, err %.3e bound %.3e"
          % (name, mode, err.max(), bound.flat[err.argmax()], (err[bound > 0] / bound[bound > 0]).max(), i[0], i[1], err[i], bound[i]))
    assert np.isfinite(sums).all()
    assert (err <= bound).all()
    assert not sums[counts[:, 1] == 0].any()                      # a class without a pixel: exactly 0


@pytest.mark.parametrize("mode", ["raw", "unit"])
@pytest.mark.parametrize("name", ["c2_s32_e300_k59", "c3_s8_e20_k33", "c4_s32_e20_k70"])
def test_class_set_accumulate_and_determinism(name, mode):
    """(b) rows outside a class set are exactly 0 (accumulate = 0) or exactly what was there (accumulate = 1); rows inside equal the
    all-classes call's bits; accumulate = 1 is first + second in one double add; two calls are bit-equal"""
    c = HC.case(name)
    full_s, full_c = _run(name, mode)
    again_s, again_c = _proto(c, c["target"], mode)
    assert np.array_equal(_bits(full_s), _bits(again_s)) and np.array_equal(full_c, again_c)
    cls = c["unseen"]
    inside = np.isin(np.arange(c["K"]), cls)
    sub_s, sub_c = _proto(c, c["target"], mode, classes=cls)
    assert np.array_equal(_bits(sub_s[inside]), _bits(full_s[inside])) and np.array_equal(sub_c[inside], full_c[inside])
    assert np.array_equal(_bits(sub_s[~inside]), _bits(np.zeros_like(sub_s[~inside]))) and not sub_c[~inside].any()
    # accumulate into something that is there: a second map (the images swapped) on top of the first call
    rng = np.random.RandomState(7)
    prev_s, prev_c = rng.randn(*full_s.shape), rng.randint(0, 1000, full_c.shape).astype(np.int64)
    acc_s, acc_c = _proto(c, c["target"], mode, classes=cls, into=(prev_s, prev_c))
    assert np.array_equal(_bits(acc_s[~inside]), _bits(prev_s[~inside])) and np.array_equal(acc_c[~inside], prev_c[~inside])
    assert np.array_equal(_bits(acc_s[inside]), _bits(prev_s[inside] + sub_s[inside])) and np.array_equal(acc_c[inside], prev_c[inside] + sub_c[inside])
    two_s, two_c = _proto(c, c["target"][::-1], mode, into=(full_s, full_c), coarse=c["coarse"][::-1])
    second_s, second_c = _proto(c, c["target"][::-1], mode, coarse=c["coarse"][::-1])
    assert np.array_equal(_bits(two_s), _bits(full_s + second_s)) and np.array_equal(two_c, full_c + second_c)


@pytest.mark.parametrize("mode", ["raw", "unit"])
@pytest.mark.parametrize("name", ["c1_s32_e5_k21", "c5_s8_e300_k59"])
def test_padded_map_gives_the_compact_maps_bits(name, mode):
    """(c) ldc > E with c0 > 0 and NaN in the padding channels"""
    c = HC.case(name)
    E, c0 = c["E"], 3
    ldc = E + 9
    padded = np.full(c["coarse"].shape[:3] + (ldc,), np.nan, dtype=np.float32)
    padded[..., c0:c0 + E] = c["coarse"]
    s, n = _proto(c, c["target"], mode, coarse=padded, ldc=ldc, c0=c0)
    full_s, full_c = _run(name, mode)
    assert np.array_equal(_bits(s), _bits(full_s)) and np.array_equal(n, full_c)


@pytest.mark.parametrize("mode", ["raw", "unit"])
@pytest.mark.parametrize("name", ["c1_s32_e5_k21", "c3_s8_e20_k33", "c6_s32_e20_k33_70x90", "c7_s8_e5_k21_70x90"])
def test_single_pixel_classes(name, mode):
    """(d) a class present at exactly one pixel gives that pixel's vector within the one-pixel bound: the corners (0,0) and (H-1,W-1)
    and a pixel on a cell border (the last row and column of a cell: y + crop = -1 mod S) -- the smallest inputs that expose a tap or
    crop error"""
    c = HC.case(name)
    S, H, W, K, E = c["S"], c["H"], c["W"], c["K"], c["E"]
    crop = HM.CROP[S]
    yb = xb = (S - 1 - crop) % S or S
    assert (yb + crop) % S == S - 1 and 0 < yb < H - 1 and 0 < xb < W - 1
    pixels = [(0, 0), (H - 1, W - 1), (yb, xb), (yb + 1, xb + 1)]
    labels = np.full((c["B"], H, W), -1, dtype=np.int64)
    b = c["B"] - 1
    for k, (y, x) in enumerate(pixels):
        labels[b, y, x] = k + 1
    sums, counts = _proto(c, labels, mode)
    s, sn, kappa = HP.pixel_vectors(c["coarse"], S, H, W)
    sabs = HM.up_crop(np.abs(c["coarse"].astype(np.float64)), S, H, W, crop)
    for k, (y, x) in enumerate(pixels):
        want = s[b, y, x] / (sn[b, y, x] if mode == "unit" else 1.0)
        A = sabs[b, y, x] / (sn[b, y, x] if mode == "unit" else 1.0)
        bound = 9 * HP.EPS * A + (HM.bound(1, kappa[b, y, x], E) if mode == "unit" else 0.0)      # <= 4 terms + 5 (n_add), + rounding of s
        err = np.abs(sums[k + 1] - want)
        print("%s %s pixel (%d,%d): max err %.3e, bound %.3e" % (name, mode, y, x, err.max(), np.min(bound)))
        assert (err <= bound).all() and tuple(counts[k + 1]) == (1, 1)
    rest = np.ones(K, dtype=bool)
    rest[1:len(pixels) + 1] = False
    assert not sums[rest].any() and not counts[rest].any()


@pytest.mark.parametrize("name", ["c1_s32_e5_k21", "c3_s8_e20_k33"])
def test_zero_region_counts_but_does_not_contribute(name):
    """(e) image 0 of the map is all zero: its pixels participate, and in UNIT mode they do not contribute; no NaN reaches sums"""
    c = HC.case(name)
    coarse = c["coarse"].copy()
    coarse[0] = 0.0
    for mode in ("unit", "raw"):
        sums, counts = _proto(c, c["target"], mode, coarse=coarse)
        ref = _reference(c, coarse, c["target"], mode)
        assert np.isfinite(sums).all() and np.array_equal(counts, ref["counts"])
        if mode == "unit":
            assert (counts[:, 0] > counts[:, 1]).any() and (counts[:, 1] > 0).any()
        npos = c["B"] * c["h"] * c["w"]
        assert (np.abs(sums - ref["sums"]) <= HP.unit_bound(ref, npos)).all()               # (RAW: ubound is 0, the RAW term alone)
    # the whole map zero: everything participates, nothing contributes, sums exactly 0
    sums, counts = _proto(c, c["target"], "unit", coarse=np.zeros_like(coarse))
    assert not sums.any() and not counts[:, 1].any() and counts[:, 0].sum() == ((c["target"] >= 0) & (c["target"] < c["K"])).sum()


@pytest.mark.parametrize("name", ["c4_s32_e20_k70", "c7_s8_e5_k21_70x90"])
def test_skipped_labels_leave_everything_untouched(name):
    """(f) labels -1 / -2 / -3 / >= K: accumulate = 0 writes zeros, accumulate = 1 leaves sums and counts as they were, bit for bit"""
    c = HC.case(name)
    K = c["K"]
    rng = np.random.RandomState(3)
    labels = rng.choice(np.array([-1, -2, -3, K, K + 5, 1 << 40], dtype=np.int64), size=c["target"].shape)
    for mode in ("raw", "unit"):
        sums, counts = _proto(c, labels, mode)
        assert np.array_equal(_bits(sums), _bits(np.zeros_like(sums))) and not counts.any()
        prev_s, prev_c = rng.randn(K, c["E"]), rng.randint(0, 99, (K, 2)).astype(np.int64)
        sums, counts = _proto(c, labels, mode, into=(prev_s, prev_c))
        assert np.array_equal(_bits(sums), _bits(prev_s)) and np.array_equal(counts, prev_c)
