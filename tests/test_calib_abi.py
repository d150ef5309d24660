"""CPU: the calibrated-stacking entry points (szn_calib_head, szn_calib_head_workspace_bytes) are declared in include/szn.h, exported
by libszn_hip.so and bound in _lib.SIGNATURES with the header's parameter lists; bad arguments are refused on the host before
anything touches a device; the Python surface (heads.calib, calib_predict, Trainer, utils.harmonic_mean_iu, train.py flags) carries the
new names, and the configurations that cannot be calibrated raise."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW = {"szn_calib_head": "int", "szn_calib_head_workspace_bytes": "size_t"}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "szn.h")).read(), flags=re.S)


def _header_params(name, res):
    m = re.search(r"\b%s\s+%s\s*\(([^)]*)\)\s*;" % (res, name), _header())
    assert m, name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def _kind(param):
    if "szn_class_set" in param:
        return "class_set"
    if param.startswith("const float* gammas"):
        return "host_floats"
    if "*" in param or param.startswith("szn_stream_t"):
        return "ptr"
    assert param.startswith("int "), param
    return "int"


def test_signatures_match_header():
    from zeroshotsemanticsegmentation_amd import _lib as L
    kinds = {L._I: "int", L._P: "ptr", L._CS: "class_set", L._FP: "host_floats"}
    for name, res in NEW.items():
        got_res, args = L.SIGNATURES[name]
        assert got_res is (L._I if res == "int" else L._SZ), name
        assert [kinds[a] for a in args] == [_kind(p) for p in _header_params(name, res)], name
    names = [p.split()[-1].lstrip("*") for p in _header_params("szn_calib_head", "int")]
    assert names == ["stride", "B", "h", "w", "E", "ldc", "c0", "H", "W", "crop", "K", "coarse", "embed", "target", "unseen", "n_gammas",
                     "gammas", "hist", "pred_index", "pred", "workspace", "stream"]
    assert [p.split()[-1] for p in _header_params("szn_calib_head_workspace_bytes", "size_t")] == ["stride", "B", "h", "w", "E", "K",
                                                                                                 "n_gammas"]
    assert re.search(r"#define\s+SZN_CALIB_MAX_GAMMAS\s+64\b", _header()) and L.CALIB_MAX_GAMMAS == 64


def test_library_exports_the_entry_points_and_refuses_bad_arguments():
    import __graft_entry__ as g
    from zeroshotsemanticsegmentation_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        g.build()
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
    lib = L.load()
    assert lib.szn_version() >= 106
    # refused on the host, before anything touches a device (the buffer only stands for non-NULL, 16-byte aligned pointers)
    raw = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p((ctypes.addressof(raw) + 15) & ~15)
    FP = ctypes.POINTER(ctypes.c_float)

    def floats(vals):
        return np.ascontiguousarray(vals, dtype=np.float32)

    def head(stride=32, K=21, gam=(-0.25, 0.0, 0.25), n=None, unseen=(2, 5), coarse=p, embed=p, target=p, hist=p, pred_index=1, pred=p,
             ws=p, crop=19, ldc=24, h=2, w=2, null_gammas=False):
        g_arr = floats(gam)
        gp = None if null_gammas else g_arr.ctypes.data_as(FP)
        return lib.szn_calib_head(stride, 1, h, w, 20, ldc, 0, 33, 47, crop, K, coarse, embed, target, L.class_set(unseen),
                                  len(g_arr) if n is None else n, gp, hist, pred_index, pred, ws, None)
    assert head(stride=16) == -1 and head(stride=0) == -1
    assert head(n=0) == -1 and head(gam=np.arange(65), n=65) == -1
    assert head(gam=(0.0, np.inf)) == -1 and head(gam=(np.nan, 0.0)) == -1 and b"finite" in lib.szn_last_error()
    assert head(gam=(0.0, 0.0)) == -1 and head(gam=(0.25, 0.0)) == -1 and b"ascending" in lib.szn_last_error()
    assert head(hist=None, pred=None) == -1
    assert head(target=None) == -1 and b"target" in lib.szn_last_error()
    assert head(pred_index=-1) == -1 and head(pred_index=3) == -1
    assert head(coarse=None) == -1 and head(embed=None) == -1 and head(ws=None) == -1 and head(null_gammas=True) == -1
    assert head(unseen=()) == -1 and b"empty" in lib.szn_last_error()
    assert head(K=3, unseen=(0, 1, 2)) == -1 and b"non-empty" in lib.szn_last_error()
    assert head(unseen=(21,)) == -1 and head(K=70, unseen=(70,)) == -1
    assert head(K=257) == -1
    assert head(ldc=19) == -1                                   # ldc < c0 + E
    assert head(w=1) == -1                                      # 47 + 19 > 32 * (1 + 1): the map cannot cover the image
    assert head(crop=64) == -1 and head(h=0) == -1
    assert head(ws=ctypes.c_void_p(p.value + 4)) == -1          # workspace not 16-byte aligned
    ws = lib.szn_calib_head_workspace_bytes
    assert ws(32, 1, 2, 2, 20, 21, 3) > 0
    assert ws(16, 1, 2, 2, 20, 21, 3) == 0 and ws(32, 1, 2, 2, 20, 21, 0) == 0 and ws(32, 1, 2, 2, 20, 21, 65) == 0
    assert ws(32, 1, 2, 2, 20, 257, 3) == 0 and ws(32, 0, 2, 2, 20, 21, 3) == 0 and ws(32, 1, 2, 0, 20, 21, 3) == 0
    sizes = [ws(8, 8, 70, 70, 300, 59, n) for n in (1, 2, 33, 64)]
    assert sizes == sorted(set(sizes))                          # grows with n_gammas ...
    assert sizes[2] - sizes[1] == 2 * 59 * 59 * 31 * 8          # ... by 2 K^2 int64 per gamma
    assert ws(8, 8, 70, 70, 300, 59, 33) >= lib.szn_fused_head_workspace_bytes(8, 70, 70, 300, 59) + 2 * 59 * 59 * 34 * 8


def test_python_surface():
    from zeroshotsemanticsegmentation_amd import heads, models, trainer_fcn, utils
    assert list(inspect.signature(heads.calib).parameters) == ["stride", "fmap", "emb", "H", "W", "unseen", "gammas", "target", "hist",
                                                              "pred_index"]
    for cls in (models.FCN32s, models.FCN8s):
        sig = inspect.signature(cls.calib_predict)
        assert list(sig.parameters) == ["self", "x", "embeddings", "unseen", "gammas", "target", "hist", "pred_index", "loss"]
        assert sig.parameters["loss"].default == "cos" and sig.parameters["pred_index"].default is None
        # the pinned parameter lists stay
        assert list(inspect.signature(cls.embed_predict).parameters) == ["self", "x", "embeddings", "target", "loss"]
        assert list(inspect.signature(cls.szn_predict).parameters) == ["self", "x", "embeddings", "unseen", "target", "group"]
        assert list(inspect.signature(cls.ms_predict).parameters) == ["self", "x", "embeddings", "scales", "flip", "target", "unseen",
                                                                      "group", "loss"]
    params = inspect.signature(trainer_fcn.Trainer.__init__).parameters
    assert list(params)[-4:] == ["calibration", "calib_sweep", "eval_scales", "eval_flip"]
    assert params["calibration"].default is None and params["calib_sweep"].default is None
    assert list(inspect.signature(utils.harmonic_mean_iu).parameters) == ["seen_metrics", "unseen_metrics"]


def test_gammas_are_checked_on_the_python_side():
    from zeroshotsemanticsegmentation_amd import _lib as L, heads
    g = heads.calib_gammas(np.linspace(-0.5, 0.5, 17))
    assert g.dtype == np.float32 and g.flags["C_CONTIGUOUS"] and g[8] == 0.0
    for bad in ([], [0.0, 0.0], [0.5, 0.0], [0.0, float("nan")], [float("inf")], list(range(65)), [1.0, 1.0 + 1e-9]):
        with pytest.raises(L.SznError):
            heads.calib_gammas(bad)


def test_parser_flags_and_refused_combinations():
    from zeroshotsemanticsegmentation_amd import train, trainer_fcn
    args = train.build_parser().parse_args(['-c', '18', '--calibration', '0.125', '--calib-sweep', '-0.25', '0.25', '5'])
    assert args.calibration == 0.125 and args.calib_sweep == [-0.25, 0.25, 5.0]
    vals = train.calib_sweep_values(args.calib_sweep)
    assert vals.dtype == np.float32 and np.array_equal(vals, np.linspace(-0.25, 0.25, 5).astype(np.float32)) and vals[2] == 0.0
    none = train.build_parser().parse_args(['-c', '18'])
    assert none.calibration is None and none.calib_sweep is None and train.calib_sweep_values(None) is None
    cfg = train.update_cfg_with_args(train.configurations[18], args)
    train.check_calibration(args.calibration, args.calib_sweep, cfg)
    train.check_calibration(None, None, dict(cfg, fcn_loss='cross_entropy', embed_dim=0))       # nothing asked: nothing refused
    for sweep in ([-0.25, 0.25, 1], [-0.25, 0.25, 65], [-0.25, 0.25, 2.5], [0.25, -0.25, 5], [0.0, 0.0, 3]):
        with pytest.raises(Exception):
            train.check_calibration(None, sweep, cfg)
    with pytest.raises(Exception):
        train.check_calibration(float("nan"), None, cfg)
    refused = [
        dict(cfg, train_unseen=[], val_unseen=[]),                       # no unseen classes
        dict(cfg, fcn_loss='cross_entropy', embed_dim=0),                # a softmax configuration
        dict(cfg, forced_unseen=True),
        dict(cfg, mode='test_all'),
    ]
    for bad in refused:
        for cal, sweep in ((0.1, None), (None, [-0.25, 0.25, 5])):
            with pytest.raises(Exception):
                train.check_calibration(cal, sweep, bad)
    with pytest.raises(Exception):
        train.check_calibration(0.1, None, cfg, eval_scales=[0.5, 1.0])
    with pytest.raises(Exception):
        train.check_calibration(0.1, None, cfg, eval_flip=True)
    # the rule both layers share, case by case
    ok = dict(has_unseen=True, embed_cfg=True, forced_unseen=False, test_all=False, eval_views=False, n_class=33, verbose_val=False)
    assert trainer_fcn.calibration_refused(**ok) is None
    for key, val in (("has_unseen", False), ("embed_cfg", False), ("forced_unseen", True), ("test_all", True), ("eval_views", True),
                     ("n_class", 257), ("verbose_val", True)):
        assert isinstance(trainer_fcn.calibration_refused(**dict(ok, **{key: val})), str), key


def test_verbose_val_is_refused(monkeypatch):
    from zeroshotsemanticsegmentation_amd import train
    cfg = train.update_cfg_with_args(train.configurations[18], train.build_parser().parse_args(['-c', '18']))
    monkeypatch.setenv("SZN_VERBOSE_VAL", "1")
    with pytest.raises(Exception):
        train.check_calibration(0.1, None, cfg)
