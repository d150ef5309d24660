"""GPU: the hard-pixel-mining head (szn_ohem_head, csrc/szn_fused_head.hip) through the C interface, on the synthetic coarse maps of
tests/helpers_calib.py: (a) conf against the float64 own-class cosine; (b) histogram, cut, counts and the relabelled target against the
exact integer restatement fed the GPU's own conf; (c) pass-through, skip set, empty images, NaN pixels, determinism; (d) conf bit-equal
to the fused cosine head's loss term on single-pixel images; (e) the fused head counts exactly the kept pixels; (f) refusals.

Shapes: helpers_calib.CASES (strides 32 / 8, E 5-300, K 21-70, 33 x 47 at B = 2, 70 x 90 at B = 1); keep 250 permille, thresh 0.0: the
threshold decides the cut in c2, c4 and c5, the budget in the others (tests/test_ohem_ref.py)."""
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
import helpers_ohem as HO  # noqa: E402
from zeroshotsemanticsegmentation_amd import _lib as L  # noqa: E402

EXTRAS = ("conf", "qhist", "cut", "counts")
SENTINEL = -7


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()           # a copy: the cached cases are read-only


def _geom(c, coarse):
    B, h, w = coarse.shape[:3]
    return c["S"], B, h, w, c["E"], c["K"]


def _ohem(c, target, keep=HO.KEEP, thresh=HO.THRESH, skip=(), drop=HO.DROP, which=EXTRAS, coarse=None, emb=None, H=None, W=None):
    """szn_ohem_head on case c (or on another map / target of its geometry) -> dict of numpy arrays: target_out and the extras"""
    lib = L.load()
    coarse = c["coarse"] if coarse is None else coarse
    S, B, h, w, E, K = _geom(c, coarse)
    H, W = H or c["H"], W or c["W"]
    cm, em, tgt = _dev(coarse), _dev(c["emb"] if emb is None else emb), _dev(target)
    assert tuple(tgt.shape) == (B, H, W)
    out = torch.full((B, H, W), SENTINEL, dtype=torch.int64, device="cuda")
    spec = dict(conf=((B, H, W), torch.float32), qhist=((B, HO.BINS), torch.int64), cut=((B,), torch.int32), counts=((B, 2), torch.int64))
    ex = {n: torch.full(spec[n][0], SENTINEL, dtype=spec[n][1], device="cuda") for n in which}
    nbytes = lib.szn_ohem_head_workspace_bytes(S, B, h, w, E, K, H, W)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    rc = lib.szn_ohem_head(S, B, h, w, E, E, 0, H, W, HM.CROP[S], K, L.ptr(cm), L.ptr(em), L.ptr(tgt), L.class_set(skip), keep, thresh,
                           drop, L.ptr(out), *([L.ptr(ex.get(n)) for n in EXTRAS] + [L.ptr(ws), L.stream_ptr()]))
    assert rc == 0, lib.szn_last_error()
    torch.cuda.synchronize()
    got = {n: t.cpu().numpy() for n, t in ex.items()}
    got["target_out"] = out.cpu().numpy()
    return got


def _cos_head(c, target, coarse=None, emb=None):
    """szn_fused_head_strided (the cosine head) -> stats (B,2) {sum of the cosines, counted pixels}"""
    lib = L.load()
    coarse = c["coarse"] if coarse is None else coarse
    S, B, h, w, E, K = _geom(c, coarse)
    H, W = target.shape[1:]
    cm, em, tgt = _dev(coarse), _dev(c["emb"] if emb is None else emb), _dev(target)
    loss, stats = torch.empty(1, device="cuda"), torch.empty(B, 2, device="cuda")
    pred = torch.empty(B, H, W, dtype=torch.int64, device="cuda")
    ws = torch.empty(lib.szn_fused_head_workspace_bytes(B, h, w, E, K), dtype=torch.uint8, device="cuda")
    rc = lib.szn_fused_head_strided(S, B, h, w, E, E, 0, H, W, HM.CROP[S], K, L.ptr(cm), L.ptr(em), L.ptr(tgt), L.ptr(loss), L.ptr(stats),
                                    L.ptr(pred), L.SZN_F32, None, L.ptr(ws), L.stream_ptr())
    assert rc == 0, lib.szn_last_error()
    torch.cuda.synchronize()
    return stats.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _run(name):
    c = HC.case(name)
    return _ohem(c, c["target"])


@pytest.mark.parametrize("name", HO.NAMES)
def test_conf_against_float64(name):
    """(a) conf is a number exactly on the evaluated pixels and lies within the project's derived bound of the float64 cosine.  (Bins are
    not compared with float64: at E = 300 up to a quarter of the pixels lie within that bound of a bin edge.)"""
    c, got, ref = HC.case(name), _run(name), HC.case_reference(name)
    ev = HO.evaluated(c["target"], c["K"])
    assert np.array_equal(~np.isnan(got["conf"]), ev)
    err = np.abs(got["conf"][ev].astype(np.float64) - HO.case_cosine(name)[ev])
    print("%s: %d evaluated, max |conf - cos64| = %.3g (bound >= %.3g)" % (name, ev.sum(), err.max(), ref["bound"][ev].min()))
    assert (err <= ref["bound"][ev]).all()


@pytest.mark.parametrize("name", HO.NAMES)
def test_histogram_cut_and_relabel_are_exact(name):
    """(b) from the GPU's own conf: qhist, cut, counts and target_out equal the integer restatement exactly; (e) the fused cosine head
    run on target_out counts exactly the kept pixels"""
    c, got = HC.case(name), _run(name)
    r = HO.select(got["conf"], c["target"], c["K"], HO.KEEP, HO.THRESH)
    assert np.array_equal(got["qhist"], r["qhist"])
    assert got["cut"].dtype == np.int32 and np.array_equal(got["cut"], r["cut"])
    assert np.array_equal(got["counts"], r["counts"])
    assert np.array_equal(got["target_out"], r["target_out"])
    assert r["dropped"].any() and (r["counts"][:, 1] >= r["keep"]).all()
    driven = (r["cut"] == 512) & (r["tmin"] < 512)
    assert driven.all() == (name in ("c2_s32_e300_k59", "c4_s32_e20_k70", "c5_s8_e300_k59")) and (driven.all() or not driven.any())
    stats = _cos_head(c, got["target_out"])
    assert np.array_equal(stats[:, 1], got["counts"][:, 1].astype(np.float32))
    # the threshold off: the budget alone decides
    off = _ohem(c, c["target"], thresh=HO.OFF)
    r = HO.select(off["conf"], c["target"], c["K"], HO.KEEP, HO.OFF)
    assert np.array_equal(off["conf"], got["conf"], equal_nan=True)
    for n in ("qhist", "cut", "counts", "target_out"):
        assert np.array_equal(off[n], r[n]), n
    assert np.array_equal(off["cut"], r["tmin"])


@pytest.mark.parametrize("name", HO.NAMES)
def test_keep_everything_returns_the_target(name):
    """(c) keep = 1000 with the threshold off: target_out == target bit for bit"""
    c = HC.case(name)
    full = _ohem(c, c["target"], keep=1000, thresh=HO.OFF, which=("counts", "cut"))
    assert np.array_equal(full["target_out"], c["target"])
    assert np.array_equal(full["counts"][:, 0], full["counts"][:, 1]) and (full["counts"][:, 0] > 0).all()
    # so does a threshold of 1: bin 1024 lies above every pixel
    top = _ohem(c, c["target"], keep=1, thresh=1.0, which=("cut",))
    assert np.array_equal(top["target_out"], c["target"]) and (top["cut"] == HO.BINS).all()


@pytest.mark.parametrize("name", ["c1_s32_e5_k21", "c3_s8_e20_k33", "c4_s32_e20_k70"])
def test_pass_through_skip_empty_image_and_nan_pixels(name):
    """(c) -1, -2, -3, labels >= K and int64 extremes come back verbatim; a skip set is neither counted nor dropped; NULL extras change
    nothing; two calls are bit-equal; an image with no valid pixel gives cut 0 and counts {0, 0}; a zeroed embedding row makes its pixels
    NaN and they are kept"""
    c = HC.case(name)
    K = c["K"]
    t = c["target"].copy()
    t[:, 10:14, 7:30] = K
    t[:, 20, :] = K + 200
    t[:, 21, :] = np.iinfo(np.int64).min
    t[:, 22, :] = np.iinfo(np.int64).max
    t[:, 23, :] = -3
    t[:, 24, :] = -4
    assert (t == -1).any() and (t == -2).any()
    a = _ohem(c, t)
    assert L.last_kernel() == "ohem_relabel_kernel" and L.prev_kernel() == "ohem_cut_kernel"
    ev = HO.evaluated(t, K)
    assert np.array_equal(a["target_out"][~ev], t[~ev]) and np.isnan(a["conf"][~ev]).all()
    r = HO.select(a["conf"], t, K, HO.KEEP, HO.THRESH)
    assert np.array_equal(a["target_out"], r["target_out"]) and np.array_equal(a["counts"], r["counts"])
    changed = a["target_out"] != t
    assert changed.any() and (a["target_out"][changed] == HO.DROP).all() and ev[changed].all()
    b = _ohem(c, t)
    for n in a:
        assert np.array_equal(a[n], b[n], equal_nan=(n == "conf")), n
    bare = _ohem(c, t, which=())
    assert np.array_equal(bare["target_out"], a["target_out"])
    # another drop label
    m5 = _ohem(c, t, drop=-5, which=())
    assert np.array_equal(m5["target_out"], np.where(changed, -5, t))
    # a skip set
    skip = c["unseen"]
    s = _ohem(c, t, skip=skip)
    in_skip = np.isin(t, skip)
    assert in_skip.any() and np.array_equal(s["target_out"][in_skip], t[in_skip]) and np.isnan(s["conf"][in_skip]).all()
    assert np.array_equal(s["counts"][:, 0], (ev & ~in_skip).reshape(c["B"], -1).sum(axis=1))
    rs = HO.select(s["conf"], t, K, HO.KEEP, HO.THRESH, skip=skip)
    for n in ("qhist", "cut", "counts", "target_out"):
        assert np.array_equal(s[n], rs[n]), n
    assert np.array_equal(s["conf"][ev & ~in_skip], a["conf"][ev & ~in_skip])
    # an image with no valid pixel
    e = t.copy()
    e[0] = np.where(ev[0], -1, t[0])
    g = _ohem(c, e)
    assert g["cut"][0] == 0 and not g["counts"][0].any() and not g["qhist"][0].any() and np.array_equal(g["target_out"][0], e[0])
    assert np.isnan(g["conf"][0]).all()
    if c["B"] > 1:
        assert np.array_equal(g["target_out"][1], a["target_out"][1]) and g["cut"][1] == a["cut"][1]
    # a zeroed embedding row: its pixels are NaN, land in bin 0 and keep their label
    emb = c["emb"].copy()
    emb[3] = 0
    z = _ohem(c, t, emb=emb)
    is3 = t == 3
    assert is3.any() and np.isnan(z["conf"][is3]).all() and (z["target_out"][is3] == 3).all()
    assert np.array_equal(z["qhist"][:, 0], is3.reshape(c["B"], -1).sum(axis=1)) and (z["cut"] >= 1).all()
    assert np.array_equal(z["counts"][:, 0], a["counts"][:, 0])
    rz = HO.select(z["conf"], t, K, HO.KEEP, HO.THRESH)
    assert np.array_equal(z["target_out"], rz["target_out"]) and np.array_equal(z["counts"], rz["counts"])


@pytest.mark.parametrize("name", ["c1_s32_e5_k21", "c2_s32_e300_k59", "c3_s8_e20_k33", "c5_s8_e300_k59"])
def test_conf_is_the_fused_heads_loss_term_bit_for_bit(name):
    """(d) B = 8 images of 33 x 47 with exactly one labelled pixel each -- the four corners, two border cells, two interior positions:
    the cosine head's per-image sum is that pixel's loss term, and it equals conf bit for bit; both strides"""
    c = HC.case(name)
    H, W, K = c["H"], c["W"], c["K"]
    assert (H, W) == (33, 47)
    spots = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, 20), (17, W - 1), (12, 13), (20, 33)]
    rng = np.random.RandomState(5)
    coarse = np.concatenate([c["coarse"]] * (8 // c["B"]), axis=0)
    coarse = (coarse * rng.uniform(0.5, 1.5, coarse.shape)).astype(np.float32)                    # eight different images
    t = np.full((8, H, W), -1, dtype=np.int64)
    for b, (y, x) in enumerate(spots):
        t[b, y, x] = rng.randint(0, K)
    got = _ohem(c, t, keep=1000, thresh=HO.OFF, coarse=coarse)
    stats = _cos_head(c, t, coarse=coarse)
    conf = np.array([got["conf"][b, y, x] for b, (y, x) in enumerate(spots)], dtype=np.float32)
    assert not np.isnan(conf).any() and np.isnan(got["conf"]).sum() == t.size - 8
    assert np.array_equal(stats[:, 1], np.ones(8, dtype=np.float32))
    assert np.array_equal(stats[:, 0].view(np.int32), conf.view(np.int32))
    assert np.array_equal(got["counts"], np.ones((8, 2), dtype=np.int64)) and np.array_equal(got["target_out"], t)


def test_launch_time_error_codes_leave_the_output_alone():
    """(f)"""
    lib = L.load()
    c = HC.case("c1_s32_e5_k21")
    cm, emb, tgt = _dev(c["coarse"]), _dev(c["emb"]), _dev(c["target"])
    ws = torch.empty(lib.szn_ohem_head_workspace_bytes(32, c["B"], c["h"], c["w"], c["E"], c["K"], c["H"], c["W"]), dtype=torch.uint8,
                     device="cuda")
    out = torch.full((c["B"], c["H"], c["W"]), SENTINEL, dtype=torch.int64, device="cuda")
    cnt = torch.full((c["B"], 2), SENTINEL, dtype=torch.int64, device="cuda")

    def head(keep=250, thresh=0.0, label=-1, skip=(), target=tgt, target_out=out, stride=32, ws=ws, crop=19):
        return lib.szn_ohem_head(stride, c["B"], c["h"], c["w"], c["E"], c["E"], 0, c["H"], c["W"], crop, c["K"], L.ptr(cm), L.ptr(emb),
                                 L.ptr(target), L.class_set(skip), keep, thresh, label, L.ptr(target_out), None, None, None, L.ptr(cnt),
                                 L.ptr(ws), L.stream_ptr())
    assert head(thresh=float("nan")) == -1 and head(thresh=float("inf")) == -1 and head(thresh=float("-inf")) == -1
    assert head(keep=0) == -1 and head(keep=1001) == -1 and head(keep=-5) == -1
    assert head(label=0) == -1 and head(label=5) == -1
    assert head(target=None) == -1 and head(target_out=None) == -1 and head(ws=None) == -1
    assert head(target_out=tgt) == -1 and b"alias" in lib.szn_last_error()
    assert head(skip=list(range(c["K"]))) == -1 and head(skip=[c["K"]]) == -1
    assert head(stride=16) == -1 and head(crop=64) == -1
    torch.cuda.synchronize()
    assert (out == SENTINEL).all().item() and (cnt == SENTINEL).all().item()
    assert torch.equal(tgt.cpu(), torch.from_numpy(np.array(c["target"])))
    assert head() == 0 and head(thresh=-2.0) == 0 and head(thresh=-1e30) == 0 and head(thresh=1e30) == 0 and head(keep=1) == 0
    assert head(keep=1000) == 0 and head(label=-3) == 0 and head(skip=[2, 5]) == 0
    assert L.last_kernel() == "ohem_relabel_kernel" and L.prev_kernel() == "ohem_cut_kernel"
    torch.cuda.synchronize()
    assert not (out == SENTINEL).any().item() and not (cnt == SENTINEL).any().item()
