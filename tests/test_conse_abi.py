"""CPU: the ConSE entry points (szn_conse_head, szn_conse_head_workspace_bytes) are declared in include/szn.h, exported by
libszn_hip.so and bound in _lib.SIGNATURES with the header's parameter lists; bad arguments are refused on the host before anything
touches a device; the Python surface (heads.conse, conse_predict, utils.conse_infer, Trainer, train.py flags) carries the new names,
and the configurations that cannot run ConSE raise."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW = {"szn_conse_head": "int", "szn_conse_head_workspace_bytes": "size_t"}


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
    names = [p.split()[-1].lstrip("*") for p in _header_params("szn_conse_head", "int")]
    assert names == ["stride", "B", "h", "w", "K", "ldc", "c0", "H", "W", "crop", "E", "coarse", "embed", "target", "unseen", "top_t",
                     "forced", "n_gammas", "gammas", "hist", "pred_index", "pred", "workspace", "stream"]
    assert [p.split()[-1] for p in _header_params("szn_conse_head_workspace_bytes", "size_t")] == ["stride", "B", "h", "w", "E", "K",
                                                                                                 "n_gammas"]
    assert re.search(r"#define\s+SZN_CONSE_MAX_TOP\s+16\b", _header()) and L.CONSE_MAX_TOP == 16


def test_library_exports_the_entry_points_and_refuses_bad_arguments():
    import __graft_entry__ as g
    from zeroshotsemanticsegmentation_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        g.build()
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
    lib = L.load()
    assert lib.szn_version() >= 113
    # refused on the host, before anything touches a device (the buffer only stands for non-NULL, 16-byte aligned pointers)
    raw = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p((ctypes.addressof(raw) + 15) & ~15)
    FP = ctypes.POINTER(ctypes.c_float)

    def floats(vals):
        return np.ascontiguousarray(vals, dtype=np.float32)

    def head(stride=32, K=21, gam=(-0.25, 0.0, 0.25), n=None, unseen=(2, 5), coarse=p, embed=p, target=p, hist=p, pred_index=1, pred=p,
             ws=p, crop=19, ldc=24, c0=0, h=2, w=2, E=20, null_gammas=False, top_t=5, forced=0):
        g_arr = floats(gam)
        gp = None if null_gammas else g_arr.ctypes.data_as(FP)
        return lib.szn_conse_head(stride, 1, h, w, K, ldc, c0, 33, 47, crop, E, coarse, embed, target, L.class_set(unseen), top_t, forced,
                                  len(g_arr) if n is None else n, gp, hist, pred_index, pred, ws, None)

    def err(word):
        return word in lib.szn_last_error()
    # szn_calib_head's refusals
    assert head(stride=16) == -1 and err(b"stride") and head(stride=0) == -1
    assert head(n=0) == -1 and err(b"n_gammas") and head(gam=np.arange(65), n=65) == -1 and err(b"n_gammas")
    assert head(gam=(0.0, np.inf)) == -1 and head(gam=(np.nan, 0.0)) == -1 and err(b"finite")
    assert head(gam=(0.0, 0.0)) == -1 and head(gam=(0.25, 0.0)) == -1 and err(b"ascending")
    assert head(hist=None, pred=None) == -1 and err(b"NULL")
    assert head(target=None) == -1 and err(b"target")
    assert head(pred_index=-1) == -1 and head(pred_index=3) == -1 and err(b"pred_index")
    assert head(coarse=None) == -1 and head(embed=None) == -1 and head(ws=None) == -1 and err(b"required")
    assert head(null_gammas=True) == -1 and err(b"gammas")
    assert head(unseen=()) == -1 and err(b"empty")
    assert head(K=3, unseen=(0, 1, 2)) == -1 and err(b"non-empty")
    assert head(unseen=(21,)) == -1 and head(K=70, ldc=70, unseen=(70,)) == -1 and err(b">= K")
    assert head(K=257, ldc=257) == -1 and err(b"SZN_MAX_CLASSES")
    assert head(w=1) == -1 and err(b"crop window")             # 47 + 19 > 32 * (1 + 1): the map cannot cover the image
    assert head(crop=64) == -1 and head(h=0) == -1 and err(b"positive") and head(E=0) == -1
    assert head(ws=ctypes.c_void_p(p.value + 4)) == -1 and err(b"aligned")
    # its own
    assert head(ldc=20) == -1 and err(b"ldc") and head(c0=4) == -1 and err(b"ldc")         # ldc < c0 + K
    assert head(top_t=0) == -1 and err(b"top_t") and head(top_t=17) == -1 and err(b"top_t") and head(top_t=-3) == -1
    assert head(forced=2) == -1 and err(b"forced") and head(forced=-1) == -1 and err(b"forced")
    assert head(forced=1) == -1 and err(b"forced")                                           # gammas with forced
    assert head(forced=1, n=0, null_gammas=True) == -1 and err(b"forced")                    # hist with forced
    assert head(forced=1, n=0, null_gammas=True, hist=None, target=None) == -1 and err(b"target")
    assert head(forced=1, n=0, null_gammas=True, hist=None, pred=None) == -1 and err(b"pred")
    assert head(forced=1, n=0, hist=None) == -1 and err(b"forced")                           # n_gammas 0 but a gammas pointer
    ws = lib.szn_conse_head_workspace_bytes
    assert ws(32, 1, 2, 2, 20, 21, 3) > 0 and ws(32, 1, 2, 2, 20, 21, 0) > 0                 # n_gammas = 0: the forced call
    assert ws(16, 1, 2, 2, 20, 21, 3) == 0 and ws(32, 1, 2, 2, 20, 21, -1) == 0 and ws(32, 1, 2, 2, 20, 21, 65) == 0
    assert ws(32, 1, 2, 2, 20, 257, 3) == 0 and ws(32, 0, 2, 2, 20, 21, 3) == 0 and ws(32, 1, 2, 0, 20, 21, 3) == 0
    assert ws(32, 1, 2, 2, 0, 21, 3) == 0
    sizes = [ws(8, 8, 70, 70, 300, 59, n) for n in (1, 2, 33, 64)]
    assert sizes == sorted(set(sizes))                          # grows with n_gammas ...
    assert sizes[2] - sizes[1] == 2 * 59 * 59 * 31 * 8          # ... by 2 K^2 int64 per gamma
    assert sizes[0] - ws(8, 8, 70, 70, 300, 59, 0) == 2 * 59 * 59 * 2 * 8
    assert ws(8, 8, 70, 70, 300, 59, 0) >= (59 * 59 + 59) * 4  # G and en
    assert ws(8, 8, 70, 70, 300, 59, 33) == ws(32, 1, 2, 2, 5, 59, 33)                       # K and n_gammas alone size it


def test_python_surface():
    from zeroshotsemanticsegmentation_amd import heads, models, trainer_fcn, utils
    sig = inspect.signature(heads.conse)
    assert list(sig.parameters) == ["stride", "fmap", "emb", "H", "W", "unseen", "top_t", "gammas", "target", "hist", "pred_index",
                                    "forced"]
    assert sig.parameters["gammas"].default is None and sig.parameters["forced"].default is False
    for cls in (models.FCN32s, models.FCN8s):
        sig = inspect.signature(cls.conse_predict)
        assert list(sig.parameters) == ["self", "x", "embeddings", "unseen", "top_t", "gammas", "target", "hist", "pred_index", "forced"]
        assert sig.parameters["forced"].default is False and sig.parameters["pred_index"].default is None
        # the pinned parameter lists stay
        assert list(inspect.signature(cls.softmax_predict).parameters) == ["self", "x", "target", "weight"]
        assert list(inspect.signature(cls.embed_predict).parameters) == ["self", "x", "embeddings", "target", "loss"]
        assert list(inspect.signature(cls.calib_predict).parameters) == ["self", "x", "embeddings", "unseen", "gammas", "target", "hist",
                                                                         "pred_index", "loss"]
    sig = inspect.signature(utils.conse_infer)
    assert list(sig.parameters) == ["score", "embeddings", "unseen", "top_t", "gamma", "target"]
    assert sig.parameters["gamma"].default == 0.0 and sig.parameters["target"].default is None
    params = inspect.signature(trainer_fcn.Trainer.__init__).parameters
    assert "conse" in params and "conse_sweep" in params
    assert list(params)[-4:] == ["calibration", "calib_sweep", "eval_scales", "eval_flip"]          # the pinned tail stays
    assert all(p.kind is p.POSITIONAL_OR_KEYWORD and p.default is not p.empty for n, p in params.items() if n.startswith("conse"))
    assert params["conse"].default is None and params["conse_sweep"].default is None
    assert list(inspect.signature(trainer_fcn.conse_refused).parameters) == ["has_unseen", "softmax_cfg", "forced_unseen", "test_all",
                                                                              "eval_views", "tuned"]


def test_top_t_is_checked_on_the_python_side():
    from zeroshotsemanticsegmentation_amd import _lib as L, heads
    assert heads.conse_top(1) == 1 and heads.conse_top(16) == 16 and heads.conse_top(np.int64(7)) == 7
    for bad in (0, 17, -1, 2.5, True):
        with pytest.raises(L.SznError):
            heads.conse_top(bad)


def test_parser_flags_and_refused_combinations():
    from zeroshotsemanticsegmentation_amd import train, trainer_fcn
    parse = train.build_parser().parse_args
    args = parse(['-c', '1', '-tu', '1,13', '-vu', '17,19', '--conse', '5', '--conse-dim', '20', '--conse-gamma', '0.125', '--conse-sweep',
                  '-0.5', '0.5', '17'])
    assert args.conse == 5 and args.conse_dim == 20 and args.conse_gamma == 0.125 and args.conse_sweep == [-0.5, 0.5, 17.0]
    none = parse(['-c', '1'])
    assert none.conse is None and none.conse_dim is None and none.conse_gamma is None and none.conse_sweep is None
    with pytest.raises(SystemExit):
        parse(['-c', '1', '--conse', '5', '--conse-dim', '7'])                 # not a width -e accepts
    cfg = train.update_cfg_with_args(train.configurations[1], args)
    assert train.check_conse(args.conse, args.conse_dim, args.conse_gamma, args.conse_sweep, cfg) == dict(top=5, dim=20, gamma=0.125)
    assert train.check_conse(10, None, None, None, cfg) == dict(top=10, dim=300, gamma=0.0)
    assert train.check_conse(None, None, None, None, cfg) is None               # nothing asked: nothing refused
    assert train.check_conse(None, None, None, None, dict(cfg, train_unseen=[], val_unseen=[])) is None
    for sat in (dict(dim=20), dict(gamma=0.1), dict(sweep=[-0.5, 0.5, 17])):    # the satellites without --conse
        with pytest.raises(Exception):
            train.check_conse(None, sat.get("dim"), sat.get("gamma"), sat.get("sweep"), cfg)
    for top in (0, 17, -2):
        with pytest.raises(Exception):
            train.check_conse(top, None, None, None, cfg)
    for gamma in (float("nan"), float("inf")):
        with pytest.raises(Exception):
            train.check_conse(5, None, gamma, None, cfg)
    for sweep in ([-0.25, 0.25, 1], [-0.25, 0.25, 65], [-0.25, 0.25, 2.5], [0.25, -0.25, 5], [0.0, 0.0, 3]):
        with pytest.raises(Exception):
            train.check_conse(5, None, None, sweep, cfg)
    emb_cfg = train.update_cfg_with_args(train.configurations[18], parse(['-c', '18']))
    refused = [
        dict(cfg, train_unseen=[], val_unseen=[]),                              # no unseen classes
        emb_cfg,                                                                # an embedding configuration
        dict(cfg, fcn_loss='cos'),
        dict(cfg, mode='test_all'),
        dict(cfg, dataset='context'),                                           # the softmax network has 21 channels
    ]
    for bad in refused:
        with pytest.raises(Exception):
            train.check_conse(5, None, None, None, bad)
    with pytest.raises(Exception):
        train.check_conse(5, None, None, None, cfg, eval_scales=[0.5, 1.0])
    with pytest.raises(Exception):
        train.check_conse(5, None, None, None, cfg, eval_flip=True)
    # -fu alone is the forced rule; with a gamma or a sweep it is refused
    fu = dict(cfg, forced_unseen=True)
    assert train.check_conse(5, None, None, None, fu) == dict(top=5, dim=300, gamma=0.0)
    with pytest.raises(Exception):
        train.check_conse(5, None, 0.1, None, fu)
    with pytest.raises(Exception):
        train.check_conse(5, None, None, [-0.5, 0.5, 17], fu)
    assert train.check_conse(5, None, None, None, dict(cfg, mode='test_fcn')) is not None
    # the rule both layers share, case by case
    ok = dict(has_unseen=True, softmax_cfg=True, forced_unseen=False, test_all=False, eval_views=False, tuned=True)
    assert trainer_fcn.conse_refused(**ok) is None
    assert trainer_fcn.conse_refused(**dict(ok, forced_unseen=True, tuned=False)) is None
    for key, val in (("has_unseen", False), ("softmax_cfg", False), ("forced_unseen", True), ("test_all", True), ("eval_views", True)):
        assert isinstance(trainer_fcn.conse_refused(**dict(ok, **{key: val})), str), key


def test_a_sweep_is_refused_with_verbose_val(monkeypatch):
    from zeroshotsemanticsegmentation_amd import train
    cfg = train.update_cfg_with_args(train.configurations[1], train.build_parser().parse_args(['-c', '1', '-tu', '1,13', '-vu', '17,19']))
    monkeypatch.setenv("SZN_VERBOSE_VAL", "1")
    assert train.check_conse(5, None, 0.1, None, cfg) is not None               # a single gamma keeps the materialised route
    with pytest.raises(Exception):
        train.check_conse(5, None, None, [-0.5, 0.5, 17], cfg)
