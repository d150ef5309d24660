"""CPU: the hubness-correction entry points (szn_hub_stats, szn_hub_head and their workspace queries) are declared in include/szn.h,
exported by libszn_hip.so and bound in _lib.SIGNATURES with the header's parameter lists; bad arguments are refused on the host before
anything touches a device; the Python surface (heads.hub_params / hub_stats / hub, hub_predict, Trainer, train.py flags) carries the new
names, and the configurations that cannot take the correction raise."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW = {"szn_hub_stats": "int", "szn_hub_stats_workspace_bytes": "size_t", "szn_hub_head": "int", "szn_hub_head_workspace_bytes": "size_t"}


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
    if param.startswith("float "):
        return "float"
    assert param.startswith("int "), param
    return "int"


def _names(name, res="int"):
    return [p.split()[-1].lstrip("*") for p in _header_params(name, res)]


def test_signatures_match_header():
    from zeroshotsemanticsegmentation_amd import _lib as L
    kinds = {L._I: "int", L._P: "ptr", L._CS: "class_set", L._FP: "host_floats", L._F: "float"}
    for name, res in NEW.items():
        got_res, args = L.SIGNATURES[name]
        assert got_res is (L._I if res == "int" else L._SZ), name
        assert [kinds[a] for a in args] == [_kind(p) for p in _header_params(name, res)], name
    assert _names("szn_hub_stats") == ["stride", "B", "h", "w", "E", "ldc", "c0", "H", "W", "crop", "K", "coarse", "embed", "target", "mode",
                                       "beta", "min_sd", "table", "sums", "counts", "workspace", "stream"]
    # szn_calib_head's arguments with the table after `unseen`
    calib = _names("szn_calib_head")
    at = calib.index("unseen") + 1
    assert _names("szn_hub_head") == calib[:at] + ["table"] + calib[at:]
    assert "const float* table" in _header_params("szn_hub_head", "int")
    assert _names("szn_hub_head_workspace_bytes", "size_t") == _names("szn_calib_head_workspace_bytes", "size_t")
    assert _names("szn_hub_stats_workspace_bytes", "size_t") == ["stride", "B", "h", "w", "E", "K"]
    text = open(os.path.join(ROOT, "include", "szn.h")).read()
    assert re.search(r"#define SZN_HUB_MEAN 0\b", text) and re.search(r"#define SZN_HUB_ZSCORE 1\b", text)
    assert L.HUB_MODES == {"mean": 0, "zscore": 1}
    # the header states the identity property and that the table may be the caller's own
    doc = text[text.index("szn_hub_stats writes"):text.index("#define SZN_HUB_MEAN")]
    assert "fmaf(sim, 1, -0.0f) == sim bit for bit" in doc and "a caller may pass one of its own" in doc
    assert "hub_table_kernel" in doc and "hub_cell_tab_kernel" in doc and "hub_stats_cell_tab_kernel" in doc


def _lib():
    import __graft_entry__ as g
    from zeroshotsemanticsegmentation_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        g.build()
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
    return L, L.load()


def test_hub_stats_refuses_bad_arguments_on_the_host():
    L, lib = _lib()
    assert lib.szn_version() >= 115
    # refused on the host, before anything touches a device (the buffer only stands for non-NULL, 16-byte aligned pointers)
    raw = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p((ctypes.addressof(raw) + 15) & ~15)

    def stats(stride=32, K=21, coarse=p, embed=p, target=p, mode=0, beta=1.0, min_sd=0.05, table=p, sums=p, counts=p, ws=p, crop=19, ldc=24,
              h=2, w=2, H=33, W=47, B=1, E=20):
        return lib.szn_hub_stats(stride, B, h, w, E, ldc, 0, H, W, crop, K, coarse, embed, target, mode, beta, min_sd, table, sums, counts,
                                 ws, None)
    for mode in (-1, 2, 7):
        assert stats(mode=mode) == -1 and b"mode" in lib.szn_last_error(), mode
    for beta in (-0.5, float("nan"), float("inf")):
        assert stats(beta=beta) == -1 and b"beta" in lib.szn_last_error(), beta
    for sd in (0.0, -1.0, float("nan"), float("inf")):
        assert stats(min_sd=sd) == -1 and b"min_sd" in lib.szn_last_error(), sd
    assert stats(table=None) == -1 and b"table" in lib.szn_last_error()
    # H * W above 2^22: a 2049 x 2048 window on a 65 x 65 map
    assert stats(H=2049, W=2048, h=65, w=65) == -1 and b"SZN_HUB_MAX_PIXELS" in lib.szn_last_error()
    # szn_fused_head_strided's
    assert stats(stride=16) == -1 and stats(stride=0) == -1
    assert stats(coarse=None) == -1 and stats(embed=None) == -1 and stats(ws=None) == -1
    assert stats(K=257) == -1 and stats(K=0) == -1 and stats(B=0) == -1 and stats(E=0) == -1 and stats(h=0) == -1
    assert stats(ldc=19) == -1                                   # ldc < c0 + E
    assert stats(w=1) == -1                                      # 47 + 19 > 32 * (1 + 1): the map cannot cover the image
    assert stats(crop=64) == -1 and stats(crop=-1) == -1 and stats(H=0) == -1
    assert stats(ws=ctypes.c_void_p(p.value + 4)) == -1          # workspace not 16-byte aligned
    assert b"hub_stats" in lib.szn_last_error()
    ws = lib.szn_hub_stats_workspace_bytes
    assert ws(32, 1, 2, 2, 20, 21) > 0 and ws(8, 2, 14, 14, 300, 59) > 0
    assert ws(16, 1, 2, 2, 20, 21) == 0 and ws(32, 1, 2, 2, 20, 257) == 0 and ws(32, 0, 2, 2, 20, 21) == 0
    # the sums (2 K int64 per image) and the counts (1 per image) follow the fused head's workspace
    assert ws(32, 3, 2, 2, 20, 21) >= lib.szn_fused_head_workspace_bytes(3, 2, 2, 20, 21) + 3 * (2 * 21 + 1) * 8


def test_hub_head_refuses_bad_arguments_on_the_host():
    L, lib = _lib()
    raw = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p((ctypes.addressof(raw) + 15) & ~15)
    FP = ctypes.POINTER(ctypes.c_float)

    def head(stride=32, K=21, gammas=(-0.25, 0.0, 0.25), n=None, unseen=(2, 5), coarse=p, embed=p, target=p, table=p, hist=p, pred_index=1,
             pred=p, ws=p, crop=19, ldc=24, h=2, w=2, null_gammas=False):
        g_arr = np.ascontiguousarray(gammas, dtype=np.float32)
        gp = None if null_gammas else g_arr.ctypes.data_as(FP)
        return lib.szn_hub_head(stride, 1, h, w, 20, ldc, 0, 33, 47, crop, K, coarse, embed, target, L.class_set(unseen), table,
                                len(g_arr) if n is None else n, gp, hist, pred_index, pred, ws, None)
    assert head(table=None) == -1 and b"table" in lib.szn_last_error()
    # szn_calib_head's
    assert head(stride=16) == -1 and head(stride=0) == -1
    assert head(n=0) == -1 and head(gammas=np.arange(65), n=65) == -1
    assert head(gammas=(0.0, np.inf)) == -1 and head(gammas=(np.nan, 0.0)) == -1 and b"finite" in lib.szn_last_error()
    assert head(gammas=(0.0, 0.0)) == -1 and head(gammas=(0.25, 0.0)) == -1 and b"ascending" in lib.szn_last_error()
    assert head(hist=None, pred=None) == -1 and b"both NULL" in lib.szn_last_error()
    assert head(target=None) == -1 and b"target" in lib.szn_last_error()
    assert head(pred_index=-1) == -1 and head(pred_index=3) == -1
    assert head(coarse=None) == -1 and head(embed=None) == -1 and head(ws=None) == -1 and head(null_gammas=True) == -1
    assert head(unseen=()) == -1 and b"empty" in lib.szn_last_error()
    assert head(K=3, unseen=(0, 1, 2)) == -1 and b"non-empty" in lib.szn_last_error()
    assert head(unseen=(21,)) == -1 and head(K=70, unseen=(70,)) == -1
    assert head(K=257) == -1
    assert head(ldc=19) == -1 and head(w=1) == -1 and head(crop=64) == -1 and head(h=0) == -1
    assert head(ws=ctypes.c_void_p(p.value + 4)) == -1
    assert b"hub_head" in lib.szn_last_error()
    ws = lib.szn_hub_head_workspace_bytes
    assert ws(32, 1, 2, 2, 20, 21, 3) > 0 and ws(16, 1, 2, 2, 20, 21, 3) == 0 and ws(32, 1, 2, 2, 20, 21, 65) == 0
    for n in (1, 33, 64):
        assert ws(8, 8, 70, 70, 300, 59, n) == lib.szn_calib_head_workspace_bytes(8, 8, 70, 70, 300, 59, n)


def test_python_surface():
    from zeroshotsemanticsegmentation_amd import _lib as L, heads, models, trainer_fcn, utils
    sig = inspect.signature(heads.hub_stats)
    assert list(sig.parameters) == ["stride", "fmap", "emb", "H", "W", "mode", "beta", "min_sd", "target", "want"]
    assert sig.parameters["target"].default is None and sig.parameters["want"].default == ()
    sig = inspect.signature(heads.hub)
    assert list(sig.parameters) == ["stride", "fmap", "emb", "H", "W", "unseen", "table", "gammas", "target", "hist", "pred_index"]
    assert all(sig.parameters[k].default is None for k in ("target", "hist", "pred_index"))
    assert heads.HUB_BETA == 1.0 and heads.HUB_MIN_SD == 0.05
    assert heads.hub_params(dict(mode="mean")) == dict(mode="mean", beta=1.0, min_sd=float(np.float32(0.05)))
    assert heads.hub_params(dict(mode="zscore", beta=0, min_sd=0.5)) == dict(mode="zscore", beta=0.0, min_sd=0.5)
    assert heads.hub_params(dict(mode="mean", beta=None, min_sd=None)) == heads.hub_params(dict(mode="mean"))
    for bad in (None, dict(), dict(beta=1.0), dict(mode="median"), dict(mode=0), dict(mode="mean", beta=-1), dict(mode="mean", beta=float("nan")),
                dict(mode="zscore", min_sd=0), dict(mode="zscore", min_sd=float("inf")), dict(mode="mean", gamma=0), dict(mode="mean", beta="x")):
        with pytest.raises(L.SznError):
            heads.hub_params(bad)
    for cls in (models.FCN32s, models.FCN8s):
        sig = inspect.signature(cls.hub_predict)
        assert list(sig.parameters) == ["self", "x", "embeddings", "unseen", "hub", "gammas", "target", "hist", "pred_index", "loss"]
        assert sig.parameters["loss"].default == "cos" and sig.parameters["pred_index"].default is None
    params = inspect.signature(trainer_fcn.Trainer.__init__).parameters
    assert params["hub"].default is None
    assert list(inspect.signature(trainer_fcn.hub_refused).parameters) == list(inspect.signature(trainer_fcn.calibration_refused).parameters)
    sig = inspect.signature(utils.hub_infer)
    assert list(sig.parameters) == ["score", "embeddings", "unseen", "mode", "beta", "gamma", "min_sd", "valid"]
    assert sig.parameters["gamma"].default == 0.0 and sig.parameters["min_sd"].default == 0.05 and sig.parameters["valid"].default is None
    assert list(inspect.signature(utils.hubness_skew).parameters) == ["hist"]


def test_parser_flags_and_refused_combinations(monkeypatch):
    from zeroshotsemanticsegmentation_amd import train, trainer_fcn
    args = train.build_parser().parse_args(['-c', '18', '--hub-correct', 'zscore', '--hub-beta', '0.5', '--hub-min-sd', '0.1'])
    assert args.hub_correct == "zscore" and args.hub_beta == 0.5 and args.hub_min_sd == 0.1
    none = train.build_parser().parse_args(['-c', '18'])
    assert none.hub_correct is None and none.hub_beta is None and none.hub_min_sd is None
    for bad in (['--hub-correct'], ['--hub-correct', 'median']):
        with pytest.raises(SystemExit):
            train.build_parser().parse_args(['-c', '18'] + bad)
    help_text = " ".join(train.build_parser().format_help().split())
    assert "--hub-correct {mean,zscore}" in help_text and "--hub-beta B" in help_text and "--hub-min-sd S" in help_text
    assert help_text.count("a default nobody has tuned") >= 2 and "An error without --hub-correct" in help_text
    cfg = train.update_cfg_with_args(train.configurations[18], args)
    assert train.check_hub("zscore", 0.5, 0.1, cfg) == dict(mode="zscore", beta=0.5, min_sd=0.1)
    assert train.check_hub("mean", None, None, cfg) == dict(mode="mean", beta=1.0, min_sd=0.05)
    assert train.check_hub(None, None, None, dict(cfg, mode='test_all')) is None           # nothing asked: nothing refused
    for beta, sd in ((0.5, None), (None, 0.1)):
        with pytest.raises(Exception, match="belong to --hub-correct"):
            train.check_hub(None, beta, sd, cfg)
    for b in (-1.0, float("nan"), float("inf")):
        with pytest.raises(Exception, match="--hub-beta: B must be finite"):
            train.check_hub("mean", b, None, cfg)
    for s in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(Exception, match="--hub-min-sd: S must be finite"):
            train.check_hub("zscore", None, s, cfg)
    refused = [
        (dict(cfg, mode='test_all'), "use -m test_fcn"),
        (dict(cfg, train_unseen=[], val_unseen=[]), "needs unseen classes"),
        (dict(cfg, fcn_loss='cross_entropy', embed_dim=0), "needs an embedding configuration"),
        (dict(cfg, forced_unseen=True), "forced_unseen"),
    ]
    for bad, why in refused:
        with pytest.raises(Exception, match="--hub-correct: .*" + why):
            train.check_hub("mean", None, None, bad)
    for kw in (dict(eval_scales=[0.5, 1.0]), dict(eval_flip=True)):
        with pytest.raises(Exception, match="eval_scales / eval_flip"):
            train.check_hub("mean", None, None, cfg, **kw)
    # the rule both layers share: calibration_refused's cases, one by one
    ok = dict(has_unseen=True, embed_cfg=True, forced_unseen=False, test_all=False, eval_views=False, n_class=33, verbose_val=False)
    assert trainer_fcn.hub_refused(**ok) is None and trainer_fcn.hub_refused(**dict(ok, n_class=256)) is None
    for key, val in (("has_unseen", False), ("embed_cfg", False), ("forced_unseen", True), ("test_all", True), ("eval_views", True),
                     ("n_class", 257), ("verbose_val", True)):
        why = trainer_fcn.hub_refused(**dict(ok, **{key: val}))
        assert isinstance(why, str) and why.startswith("the hubness correction") and "calibration" not in why, key
        assert trainer_fcn.calibration_refused(**dict(ok, **{key: val})) is not None, key
    monkeypatch.setenv("SZN_VERBOSE_VAL", "1")
    with pytest.raises(Exception, match="SZN_VERBOSE_VAL"):
        train.check_hub("mean", None, None, cfg)
