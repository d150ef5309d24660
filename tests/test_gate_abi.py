"""CPU: the soft-gate entry points (szn_soft_gate_head, szn_soft_gate_head_tabled, szn_soft_gate_head_workspace_bytes) are declared in
include/szn.h, exported by libszn_hip.so and bound in _lib.SIGNATURES with the header's parameter lists; bad arguments are refused on the
host before anything touches a device; the Python surface (heads.soft_gate, seen_gate_predict, Trainer, train.py flags) carries the new
names, and the configurations that cannot take the gate raise."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW = {"szn_soft_gate_head": "int", "szn_soft_gate_head_tabled": "int", "szn_soft_gate_head_workspace_bytes": "size_t"}


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
    if param.startswith("float "):
        return "float"
    assert param.startswith("int "), param
    return "int"


def test_signatures_match_header():
    from zeroshotsemanticsegmentation_amd import _lib as L
    kinds = {L._I: "int", L._P: "ptr", L._CS: "class_set", L._FP: "host_floats", L._F: "float"}
    for name, res in NEW.items():
        got_res, args = L.SIGNATURES[name]
        assert got_res is (L._I if res == "int" else L._SZ), name
        assert [kinds[a] for a in args] == [_kind(p) for p in _header_params(name, res)], name
    assert _header_params("szn_soft_gate_head_tabled", "int") == _header_params("szn_soft_gate_head", "int")
    names = [p.split()[-1].lstrip("*") for p in _header_params("szn_soft_gate_head", "int")]
    assert names == ["stride", "B", "h", "w", "E", "ldc", "c0", "H", "W", "crop", "K", "coarse", "embed", "target", "unseen", "margin",
                     "temperature", "weight", "n_taus", "taus", "hist", "pred_index", "pred", "eff", "workspace", "stream"]
    # the sweep's arguments with temperature and weight after the margin and eff after pred
    sweep = [p.split()[-1].lstrip("*") for p in _header_params("szn_seen_sweep_head", "int")]
    assert [n for n in names if n not in ("temperature", "weight", "eff")] == sweep
    assert [p.split()[-1] for p in _header_params("szn_soft_gate_head_workspace_bytes", "size_t")] == ["stride", "B", "h", "w", "E", "K",
                                                                                                     "n_taus"]
    # the header states how the two candidates differ from the sweep's
    text = open(os.path.join(ROOT, "include", "szn.h")).read()
    doc = text[text.index("szn_soft_gate_head:"):text.index("size_t szn_soft_gate_head_workspace_bytes")]
    assert "TRUE argmax" in doc and "zeroed-row" in doc and "NOT szn_seen_sweep_head's pair" in doc


def test_library_exports_the_entry_points_and_refuses_bad_arguments():
    import __graft_entry__ as g
    from zeroshotsemanticsegmentation_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        g.build()
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
    lib = L.load()
    assert lib.szn_version() >= 114
    # refused on the host, before anything touches a device (the buffer only stands for non-NULL, 16-byte aligned pointers)
    raw = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p((ctypes.addressof(raw) + 15) & ~15)
    FP = ctypes.POINTER(ctypes.c_float)

    def head(stride=32, K=21, taus=(-0.25, 0.0, 0.25), n=None, unseen=(2, 5), coarse=p, embed=p, target=p, margin=p, hist=p, pred_index=1,
             pred=p, eff=p, ws=p, crop=19, ldc=24, h=2, w=2, null_taus=False, temperature=0.1, weight=1.0):
        t_arr = np.ascontiguousarray(taus, dtype=np.float32)
        tp = None if null_taus else t_arr.ctypes.data_as(FP)
        args = (stride, 1, h, w, 20, ldc, 0, 33, 47, crop, K, coarse, embed, target, L.class_set(unseen), margin, temperature, weight,
                len(t_arr) if n is None else n, tp, hist, pred_index, pred, eff, ws, None)
        rc = lib.szn_soft_gate_head(*args)
        assert lib.szn_soft_gate_head_tabled(*args) == rc          # the same refusals
        return rc
    # the gate's own refusals
    for t in (0.0, -0.1, float("nan"), float("inf")):
        assert head(temperature=t) == -1 and b"temperature" in lib.szn_last_error(), t
    for wgt in (-1.0, float("nan"), float("inf")):
        assert head(weight=wgt) == -1 and b"weight" in lib.szn_last_error(), wgt
    assert head(hist=None, pred=None, eff=None) == -1 and b"all NULL" in lib.szn_last_error()
    # the sweep's
    assert head(stride=16) == -1 and head(stride=0) == -1
    assert head(n=0) == -1 and head(taus=np.arange(65), n=65) == -1
    assert head(taus=(0.0, np.inf)) == -1 and head(taus=(np.nan, 0.0)) == -1 and b"finite" in lib.szn_last_error()
    assert head(taus=(0.0, 0.0)) == -1 and head(taus=(0.25, 0.0)) == -1 and b"ascending" in lib.szn_last_error()
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
    assert b"soft_gate_head" in lib.szn_last_error()
    ws = lib.szn_soft_gate_head_workspace_bytes
    assert ws(32, 1, 2, 2, 20, 21, 3) > 0
    assert ws(16, 1, 2, 2, 20, 21, 3) == 0 and ws(32, 1, 2, 2, 20, 21, 0) == 0 and ws(32, 1, 2, 2, 20, 21, 65) == 0
    assert ws(32, 1, 2, 2, 20, 257, 3) == 0 and ws(32, 0, 2, 2, 20, 21, 3) == 0
    for n in (1, 33, 64):
        assert ws(8, 8, 70, 70, 300, 59, n) == lib.szn_seen_sweep_head_workspace_bytes(8, 8, 70, 70, 300, 59, n)


def test_python_surface():
    from zeroshotsemanticsegmentation_amd import _lib as L, heads, models, trainer_fcn, utils
    sig = inspect.signature(heads.soft_gate)
    assert list(sig.parameters) == ["stride", "fmap", "emb", "H", "W", "unseen", "margin", "taus", "temperature", "weight", "target", "hist",
                                    "pred_index", "want_eff", "ws"]
    assert all(sig.parameters[k].default is None for k in ("target", "hist", "pred_index", "ws")) and sig.parameters["want_eff"].default is False
    assert list(inspect.signature(heads.soft_gate_workspace_bytes).parameters) == ["stride", "fmap", "emb", "n_taus"]
    assert heads.GATE_TEMPERATURE == 0.1
    assert heads.gate_params(dict(weight=2)) == (2.0, float(np.float32(0.1)))
    assert heads.gate_params(dict(weight=0, temperature=0.5)) == (0.0, 0.5)
    for bad in (None, dict(), dict(temperature=0.1), dict(weight=-1), dict(weight=float("nan")), dict(weight=1, temperature=0),
                dict(weight=1, temperature=float("inf")), dict(weight=1, tau=0), dict(weight="x")):
        with pytest.raises(L.SznError):
            heads.gate_params(bad)
    for cls in (models.FCN32s, models.FCN8s):
        sig = inspect.signature(cls.seen_gate_predict)
        assert list(sig.parameters) == ["self", "x", "embeddings", "unseen", "taus", "gate", "target", "hist", "pred_index", "loss"]
        assert sig.parameters["loss"].default == "cos" and sig.parameters["pred_index"].default is None
    params = inspect.signature(trainer_fcn.Trainer.__init__).parameters
    assert params["seen_gate"].default is None
    assert list(inspect.signature(trainer_fcn.seen_gate_refused).parameters) == list(
        inspect.signature(trainer_fcn.seen_threshold_refused).parameters)
    assert list(inspect.signature(utils.soft_gate_infer).parameters) == ["score", "seen_mask_score", "embeddings", "unseen", "tau",
                                                                         "temperature", "weight"]


def test_parser_flags_and_refused_combinations(monkeypatch):
    from zeroshotsemanticsegmentation_amd import train, trainer_fcn
    args = train.build_parser().parse_args(['-c', '18', '-m', 'test_all', '--seen-gate', '1.5', '--gate-temperature', '0.05'])
    assert args.seen_gate == 1.5 and args.gate_temperature == 0.05
    none = train.build_parser().parse_args(['-c', '18'])
    assert none.seen_gate is None and none.gate_temperature is None
    with pytest.raises(SystemExit):
        train.build_parser().parse_args(['-c', '18', '--seen-gate'])                       # WEIGHT has no default
    help_text = " ".join(train.build_parser().format_help().split())
    assert "--seen-gate WEIGHT" in help_text and "--gate-temperature T" in help_text
    assert "Default 0.1: a hyper-parameter default, not a tuned value. An error without --seen-gate" in help_text
    cfg = train.update_cfg_with_args(train.configurations[18], args)
    assert train.check_seen_gate(1.5, 0.05, cfg) == dict(weight=1.5, temperature=0.05)
    assert train.check_seen_gate(0.0, None, cfg) == dict(weight=0.0, temperature=0.1)
    assert train.check_seen_gate(None, None, dict(cfg, mode='train')) is None              # nothing asked: nothing refused
    with pytest.raises(Exception, match="--gate-temperature: belongs to --seen-gate"):
        train.check_seen_gate(None, 0.1, cfg)
    for w in (-1.0, float("nan"), float("inf")):
        with pytest.raises(Exception, match="--seen-gate: WEIGHT must be finite"):
            train.check_seen_gate(w, None, cfg)
    for t in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(Exception, match="--gate-temperature: T must be finite"):
            train.check_seen_gate(1.0, t, cfg)
    refused = [
        (dict(cfg, mode='train'), "full SZN network only"), (dict(cfg, mode='test_fcn'), "full SZN network only"),
        (dict(cfg, train_unseen=[], val_unseen=[]), "needs unseen classes"),
        (dict(cfg, fcn_loss='cross_entropy', embed_dim=0), "needs an embedding configuration"),
        (dict(cfg, forced_unseen=True), "forced_unseen"),
    ]
    for bad, why in refused:
        with pytest.raises(Exception, match="--seen-gate: .*" + why):
            train.check_seen_gate(1.0, None, bad)
    for kw, why in ((dict(calibration=0.1), "not together with --calibration"), (dict(calib_sweep=[-0.25, 0.25, 5]), "not together with"),
                    (dict(eval_scales=[0.5, 1.0]), "eval_scales / eval_flip"), (dict(eval_flip=True), "eval_scales / eval_flip")):
        with pytest.raises(Exception, match=why):
            train.check_seen_gate(1.0, None, cfg, **kw)
    # the rule both layers share: seen_threshold_refused's reasons, case by case
    ok = dict(has_unseen=True, embed_cfg=True, forced_unseen=False, test_all=True, eval_views=False, n_class=33, verbose_val=False)
    assert trainer_fcn.seen_gate_refused(**ok) is None and trainer_fcn.seen_gate_refused(**dict(ok, n_class=256)) is None
    for key, val in (("has_unseen", False), ("embed_cfg", False), ("forced_unseen", True), ("test_all", False), ("eval_views", True),
                     ("n_class", 257), ("verbose_val", True)):
        why = trainer_fcn.seen_gate_refused(**dict(ok, **{key: val}))
        thr = trainer_fcn.seen_threshold_refused(**dict(ok, **{key: val}))
        assert isinstance(why, str) and "soft seen/unseen gate" in why, key
        assert why == thr.replace("a seen-mask threshold", "the soft seen/unseen gate"), key
    monkeypatch.setenv("SZN_VERBOSE_VAL", "1")
    with pytest.raises(Exception, match="SZN_VERBOSE_VAL"):
        train.check_seen_gate(1.0, None, cfg)
