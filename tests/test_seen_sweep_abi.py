"""CPU: the seen-mask threshold entry points (szn_seenmask_margin, szn_seen_sweep_head, szn_seen_sweep_head_workspace_bytes) are
declared in include/szn.h, exported by libszn_hip.so and bound in _lib.SIGNATURES with the header's parameter lists; bad arguments are
refused on the host before anything touches a device; the Python surface (heads.seenmask_margin / seen_sweep, seen_sweep_predict,
Trainer, train.py flags) carries the new names, and the configurations that cannot take a threshold raise."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW = {"szn_seenmask_margin": "int", "szn_seen_sweep_head": "int", "szn_seen_sweep_head_tabled": "int",
       "szn_seen_sweep_head_workspace_bytes": "size_t"}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "szn.h")).read(), flags=re.S)


def _header_params(name, res):
    m = re.search(r"\b%s\s+%s\s*\(([^)]*)\)\s*;" % (res, name), _header())
    assert m, name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def _kind(param):
    if "szn_class_set" in param:
        return "class_set"
    if param.startswith("const float* taus"):
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
    assert _header_params("szn_seen_sweep_head_tabled", "int") == _header_params("szn_seen_sweep_head", "int")
    names = [p.split()[-1].lstrip("*") for p in _header_params("szn_seen_sweep_head", "int")]
    assert names == ["stride", "B", "h", "w", "E", "ldc", "c0", "H", "W", "crop", "K", "coarse", "embed", "target", "unseen", "margin",
                     "n_taus", "taus", "hist", "pred_index", "pred", "workspace", "stream"]
    assert [p.split()[-1] for p in _header_params("szn_seen_sweep_head_workspace_bytes", "size_t")] == ["stride", "B", "h", "w", "E", "K",
                                                                                                      "n_taus"]
    names = [p.split()[-1].lstrip("*") for p in _header_params("szn_seenmask_margin", "int")]
    assert names == ["B", "h", "w", "ldc", "c0", "H", "W", "crop", "coarse", "weight", "margin", "stream"]
    assert re.search(r"#define\s+SZN_SEEN_SWEEP_MAX_TAUS\s+64\b", _header()) and L.SEEN_SWEEP_MAX_TAUS == 64


def test_library_exports_the_entry_points_and_refuses_bad_arguments():
    import __graft_entry__ as g
    from zeroshotsemanticsegmentation_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        g.build()
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
    lib = L.load()
    assert lib.szn_version() >= 109
    # refused on the host, before anything touches a device (the buffer only stands for non-NULL, 16-byte aligned pointers)
    raw = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p((ctypes.addressof(raw) + 15) & ~15)
    FP = ctypes.POINTER(ctypes.c_float)

    def floats(vals):
        return np.ascontiguousarray(vals, dtype=np.float32)

    def head(stride=32, K=21, taus=(-0.25, 0.0, 0.25), n=None, unseen=(2, 5), coarse=p, embed=p, target=p, margin=p, hist=p, pred_index=1,
             pred=p, ws=p, crop=19, ldc=24, h=2, w=2, null_taus=False):
        t_arr = floats(taus)
        tp = None if null_taus else t_arr.ctypes.data_as(FP)
        args = (stride, 1, h, w, 20, ldc, 0, 33, 47, crop, K, coarse, embed, target, L.class_set(unseen), margin,
                len(t_arr) if n is None else n, tp, hist, pred_index, pred, ws, None)
        rc = lib.szn_seen_sweep_head(*args)
        assert lib.szn_seen_sweep_head_tabled(*args) == rc          # the same refusals
        return rc
    assert head(stride=16) == -1 and head(stride=0) == -1
    assert head(n=0) == -1 and head(taus=np.arange(65), n=65) == -1
    assert head(taus=(0.0, np.inf)) == -1 and head(taus=(np.nan, 0.0)) == -1 and b"finite" in lib.szn_last_error()
    assert head(taus=(0.0, 0.0)) == -1 and head(taus=(0.25, 0.0)) == -1 and b"ascending" in lib.szn_last_error()
    assert head(hist=None, pred=None) == -1
    assert head(target=None) == -1 and b"target" in lib.szn_last_error()
    assert head(pred_index=-1) == -1 and head(pred_index=3) == -1
    assert head(coarse=None) == -1 and head(embed=None) == -1 and head(ws=None) == -1 and head(null_taus=True) == -1
    assert head(margin=None) == -1 and b"margin" in lib.szn_last_error()
    assert head(unseen=()) == -1 and b"empty" in lib.szn_last_error()
    assert head(K=3, unseen=(0, 1, 2)) == -1 and b"non-empty" in lib.szn_last_error()
    assert head(unseen=(21,)) == -1 and head(K=70, unseen=(70,)) == -1
    assert head(K=257) == -1
    assert head(ldc=19) == -1                                   # ldc < c0 + E
    assert head(w=1) == -1                                      # 47 + 19 > 32 * (1 + 1): the map cannot cover the image
    assert head(crop=64) == -1 and head(h=0) == -1
    assert head(ws=ctypes.c_void_p(p.value + 4)) == -1          # workspace not 16-byte aligned
    assert b"seen_sweep_head" in lib.szn_last_error()
    ws = lib.szn_seen_sweep_head_workspace_bytes
    assert ws(32, 1, 2, 2, 20, 21, 3) > 0
    assert ws(16, 1, 2, 2, 20, 21, 3) == 0 and ws(32, 1, 2, 2, 20, 21, 0) == 0 and ws(32, 1, 2, 2, 20, 21, 65) == 0
    assert ws(32, 1, 2, 2, 20, 257, 3) == 0 and ws(32, 0, 2, 2, 20, 21, 3) == 0 and ws(32, 1, 2, 0, 20, 21, 3) == 0
    sizes = [ws(8, 8, 70, 70, 300, 59, n) for n in (1, 2, 33, 64)]
    assert sizes == sorted(set(sizes))                          # grows with n_taus ...
    assert sizes[1] - sizes[0] == 2 * 59 * 59 * 8               # ... by 2 K^2 int64 per tau
    assert sizes[2] - sizes[1] == 2 * 59 * 59 * 31 * 8 and sizes[3] - sizes[2] == 2 * 59 * 59 * 31 * 8
    assert all(s % 16 == 0 for s in sizes)
    assert ws(8, 8, 70, 70, 300, 59, 33) >= lib.szn_fused_head_workspace_bytes(8, 70, 70, 300, 59) + 2 * 59 * 59 * 34 * 8
    assert ws(8, 8, 70, 70, 300, 59, 33) == lib.szn_calib_head_workspace_bytes(8, 8, 70, 70, 300, 59, 33)

    # the margin: szn_seenmask_head_k's geometry checks, and its three pointers
    def margin(B=1, h=2, w=2, H=33, W=47, crop=19, coarse=p, weight=p, out=p):
        return lib.szn_seenmask_margin(B, h, w, 2, 0, H, W, crop, coarse, weight, out, None)
    assert margin(B=0) == -1 and margin(h=0) == -1 and margin(w=0) == -1 and margin(H=0) == -1 and margin(W=0) == -1
    assert margin(crop=-1) == -1
    assert margin(coarse=None) == -1 and margin(weight=None) == -1 and margin(out=None) == -1 and b"null" in lib.szn_last_error()
    assert margin(w=1, W=47) == -1 and b"does not fit" in lib.szn_last_error()       # (19 + 46) >> 5 = 2 > 1
    assert margin(h=1, H=50) == -1


def test_python_surface():
    from zeroshotsemanticsegmentation_amd import heads, models, trainer_fcn
    assert list(inspect.signature(heads.seenmask_margin).parameters) == ["coarse", "E", "up_w", "H", "W"]
    assert list(inspect.signature(heads.seen_sweep_taus).parameters) == ["taus"]
    sig = inspect.signature(heads.seen_sweep)
    assert list(sig.parameters) == ["stride", "fmap", "emb", "H", "W", "unseen", "margin", "taus", "target", "hist", "pred_index", "ws"]
    assert all(sig.parameters[k].default is None for k in ("target", "hist", "pred_index", "ws"))
    for cls in (models.FCN32s, models.FCN8s):
        sig = inspect.signature(cls.seen_sweep_predict)
        assert list(sig.parameters) == ["self", "x", "embeddings", "unseen", "taus", "target", "hist", "pred_index", "loss"]
        assert sig.parameters["loss"].default == "cos" and sig.parameters["pred_index"].default is None
        # the pinned parameter lists stay
        assert list(inspect.signature(cls.embed_predict).parameters) == ["self", "x", "embeddings", "target", "loss"]
        for name in ("szn_predict", "szn_predict_mse", "szn_predict_sim_ce"):
            assert list(inspect.signature(getattr(cls, name)).parameters) == ["self", "x", "embeddings", "unseen", "target", "group"]
        assert list(inspect.signature(cls.ms_predict).parameters) == ["self", "x", "embeddings", "scales", "flip", "target", "unseen",
                                                                      "group", "loss"]
        assert list(inspect.signature(cls.calib_predict).parameters) == ["self", "x", "embeddings", "unseen", "gammas", "target", "hist",
                                                                         "pred_index", "loss"]
    params = inspect.signature(trainer_fcn.Trainer.__init__).parameters
    names = list(params)
    assert names[-4:] == ["calibration", "calib_sweep", "eval_scales", "eval_flip"]
    i = names.index("augment")
    assert names[i + 1:i + 3] == ["seen_threshold", "seen_sweep"]
    assert params["seen_threshold"].default is None and params["seen_sweep"].default is None
    j = names.index("pseudo_start_epoch")
    assert names[j:j + 4] == ["pseudo_start_epoch", "ohem", "ohem_start_epoch", "calibration"]
    assert list(inspect.signature(trainer_fcn.seen_threshold_refused).parameters) == ["has_unseen", "embed_cfg", "forced_unseen",
                                                                                    "test_all", "eval_views", "n_class", "verbose_val"]


def test_taus_are_checked_on_the_python_side():
    from zeroshotsemanticsegmentation_amd import _lib as L, heads
    t = heads.seen_sweep_taus(np.linspace(-2, 2, 17))
    assert t.dtype == np.float32 and t.flags["C_CONTIGUOUS"] and t[8] == 0.0
    assert heads.seen_sweep_taus([0.5]).tolist() == [0.5] and heads.seen_sweep_taus(np.arange(64)).size == 64
    for bad in ([], [0.0, 0.0], [0.5, 0.0], [0.0, float("nan")], [float("inf")], list(range(65)), [1.0, 1.0 + 1e-9]):
        with pytest.raises(L.SznError):
            heads.seen_sweep_taus(bad)


def test_parser_flags_and_refused_combinations():
    from zeroshotsemanticsegmentation_amd import train, trainer_fcn
    args = train.build_parser().parse_args(['-c', '18', '-m', 'test_all', '--seen-threshold', '0.5', '--seen-sweep', '-2', '2', '5'])
    assert args.seen_threshold == 0.5 and args.seen_sweep == [-2.0, 2.0, 5.0]
    vals = train.seen_sweep_values(args.seen_sweep)
    assert vals.dtype == np.float32 and np.array_equal(vals, np.linspace(-2, 2, 5).astype(np.float32)) and vals[2] == 0.0
    none = train.build_parser().parse_args(['-c', '18'])
    assert none.seen_threshold is None and none.seen_sweep is None and train.seen_sweep_values(None) is None
    help_text = train.build_parser().format_help()
    assert "logit" in help_text and "sigmoid(TAU)" in help_text
    cfg = train.update_cfg_with_args(train.configurations[18], args)
    assert cfg['mode'] == 'test_all'
    train.check_seen_threshold(args.seen_threshold, args.seen_sweep, cfg)
    train.check_seen_threshold(None, None, dict(cfg, mode='train', fcn_loss='cross_entropy', embed_dim=0))    # nothing asked: nothing refused
    for sweep in ([-2, 2, 1], [-2, 2, 65], [-2, 2, 2.5], [2, -2, 5], [0.0, 0.0, 3]):
        with pytest.raises(Exception, match="--seen-sweep: "):
            train.check_seen_threshold(None, sweep, cfg)
    for tau in (float("nan"), float("inf")):
        with pytest.raises(Exception, match="--seen-threshold: TAU must be finite"):
            train.check_seen_threshold(tau, None, cfg)
    refused = [
        (dict(cfg, mode='train'), "full SZN network only"), (dict(cfg, mode='test_fcn'), "full SZN network only"),
        (dict(cfg, train_unseen=[], val_unseen=[]), "needs unseen classes"),
        (dict(cfg, fcn_loss='cross_entropy', embed_dim=0), "needs an embedding configuration"),
        (dict(cfg, forced_unseen=True), "forced_unseen"),
    ]
    for bad, why in refused:
        for tau, sweep in ((0.5, None), (None, [-2, 2, 5])):
            with pytest.raises(Exception, match="--seen-threshold / --seen-sweep: .*" + why):
                train.check_seen_threshold(tau, sweep, bad)
    for kw, why in ((dict(calibration=0.1), "not together with --calibration"), (dict(calib_sweep=[-0.25, 0.25, 5]), "not together with"),
                    (dict(eval_scales=[0.5, 1.0]), "eval_scales / eval_flip"), (dict(eval_flip=True), "eval_scales / eval_flip")):
        with pytest.raises(Exception, match=why):
            train.check_seen_threshold(0.5, None, cfg, **kw)
    # the rule both layers share, case by case
    ok = dict(has_unseen=True, embed_cfg=True, forced_unseen=False, test_all=True, eval_views=False, n_class=33, verbose_val=False)
    assert trainer_fcn.seen_threshold_refused(**ok) is None
    assert trainer_fcn.seen_threshold_refused(**dict(ok, n_class=256)) is None
    for key, val in (("has_unseen", False), ("embed_cfg", False), ("forced_unseen", True), ("test_all", False), ("eval_views", True),
                     ("n_class", 257), ("verbose_val", True)):
        assert isinstance(trainer_fcn.seen_threshold_refused(**dict(ok, **{key: val})), str), key


def test_verbose_val_is_refused(monkeypatch):
    from zeroshotsemanticsegmentation_amd import train
    args = train.build_parser().parse_args(['-c', '18', '-m', 'test_all'])
    cfg = train.update_cfg_with_args(train.configurations[18], args)
    train.check_seen_threshold(0.5, None, cfg)
    monkeypatch.setenv("SZN_VERBOSE_VAL", "1")
    with pytest.raises(Exception, match="SZN_VERBOSE_VAL"):
        train.check_seen_threshold(0.5, None, cfg)
