"""CPU: the pseudo-label entry points (szn_pseudo_head, szn_pseudo_head_workspace_bytes) are declared in include/szn.h, exported by
libszn_hip.so and bound in _lib.SIGNATURES with the header's parameter lists; bad arguments are refused on the host before anything
touches a device; the Python surface (heads.pseudo, TrainStep(pseudo=), Trainer(pseudo=, pseudo_start_epoch=), the datasets' hide_unseen
keyword, train.py flags) carries the new names, and the configurations that cannot self-train raise."""
import ctypes
import inspect
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW = {"szn_pseudo_head": "int", "szn_pseudo_head_workspace_bytes": "size_t"}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "szn.h")).read(), flags=re.S)


def _header_params(name, res):
    m = re.search(r"\b%s\s+%s\s*\(([^)]*)\)\s*;" % (res, name), _header())
    assert m, name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def _kind(param):
    if "szn_class_set" in param:
        return "class_set"
    if "*" in param or param.startswith("szn_stream_t"):
        return "ptr"
    if param.startswith("float "):
        return "float"
    if param.startswith("int64_t "):
        return "int64"
    assert param.startswith("int "), param
    return "int"


def test_signatures_match_header():
    from zeroshotsemanticsegmentation_amd import _lib as L
    kinds = {L._I: "int", L._P: "ptr", L._CS: "class_set", L._F: "float", L._I64: "int64"}
    for name, res in NEW.items():
        got_res, args = L.SIGNATURES[name]
        assert got_res is (L._I if res == "int" else L._SZ), name
        assert [kinds[a] for a in args] == [_kind(p) for p in _header_params(name, res)], name
    names = [p.split()[-1].lstrip("*") for p in _header_params("szn_pseudo_head", "int")]
    assert names == ["stride", "B", "h", "w", "E", "ldc", "c0", "H", "W", "crop", "K", "coarse", "embed", "target", "unseen", "gamma",
                     "conf_floor", "keep_permille", "cand_label", "target_out", "cand", "conf", "qhist", "thr", "counts", "workspace",
                     "stream"]
    assert [p.split()[-1] for p in _header_params("szn_pseudo_head_workspace_bytes", "size_t")] == ["stride", "B", "h", "w", "E", "K",
                                                                                                  "H", "W"]
    assert re.search(r"#define\s+SZN_PSEUDO_BINS\s+1024\b", _header()) and L.PSEUDO_BINS == 1024


def test_library_exports_the_entry_points_and_refuses_bad_arguments():
    import __graft_entry__ as g
    from zeroshotsemanticsegmentation_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        g.build()
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
    lib = L.load()
    assert lib.szn_version() >= 107
    # refused on the host, before anything touches a device (the buffers only stand for non-NULL, 16-byte aligned pointers)
    raw, raw2 = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
    p = ctypes.c_void_p((ctypes.addressof(raw) + 15) & ~15)
    q = ctypes.c_void_p((ctypes.addressof(raw2) + 15) & ~15)

    def head(stride=32, K=21, gamma=0.0, floor=0.2, keep=300, label=-3, unseen=(2, 5), coarse=p, embed=p, target=p, out=q, ws=p, crop=19,
             ldc=24, h=2, w=2):
        return lib.szn_pseudo_head(stride, 1, h, w, 20, ldc, 0, 33, 47, crop, K, coarse, embed, target, L.class_set(unseen), gamma, floor,
                                   keep, label, out, None, None, None, None, None, ws, None)
    # szn_calib_head's refusals of the shared arguments
    assert head(stride=16) == -1 and head(stride=0) == -1
    assert head(coarse=None) == -1 and head(embed=None) == -1 and head(ws=None) == -1
    assert head(unseen=()) == -1 and b"empty" in lib.szn_last_error()
    assert head(K=3, unseen=(0, 1, 2)) == -1 and b"non-empty" in lib.szn_last_error()
    assert head(unseen=(21,)) == -1 and head(K=70, unseen=(70,)) == -1
    assert head(K=257) == -1
    assert head(ldc=19) == -1                                   # ldc < c0 + E
    assert head(w=1) == -1                                      # 47 + 19 > 32 * (1 + 1): the map cannot cover the image
    assert head(crop=64) == -1 and head(h=0) == -1
    assert head(ws=ctypes.c_void_p(p.value + 4)) == -1          # workspace not 16-byte aligned
    # its own
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert head(gamma=bad) == -1 and b"finite" in lib.szn_last_error()
        assert head(floor=bad) == -1 and b"finite" in lib.szn_last_error()
    assert head(keep=0) == -1 and head(keep=1001) == -1 and head(keep=-1) == -1 and b"keep_permille" in lib.szn_last_error()
    assert head(label=0) == -1 and head(label=7) == -1 and b"cand_label" in lib.szn_last_error()
    assert head(target=None) == -1 and head(out=None) == -1
    assert head(out=p) == -1 and b"alias" in lib.szn_last_error()
    ws = lib.szn_pseudo_head_workspace_bytes
    assert ws(32, 1, 2, 2, 20, 21, 33, 47) > 0
    assert ws(16, 1, 2, 2, 20, 21, 33, 47) == 0 and ws(32, 1, 2, 2, 20, 257, 33, 47) == 0 and ws(32, 0, 2, 2, 20, 21, 33, 47) == 0
    assert ws(32, 1, 2, 0, 20, 21, 33, 47) == 0 and ws(32, 1, 2, 2, 20, 21, 0, 47) == 0 and ws(32, 1, 2, 2, 20, 21, 33, 0) == 0
    # the fused head's workspace + the [K][1024] table + thresholds + 8 bytes per pixel
    base = lib.szn_fused_head_workspace_bytes(8, 70, 70, 300, 59)
    got = ws(8, 8, 70, 70, 300, 59, 512, 512)
    assert base + 59 * 1024 * 8 + 59 * 4 + 8 * 512 * 512 * 8 <= got <= base + 59 * 1024 * 8 + 59 * 4 + 8 * 512 * 512 * 8 + 1024
    assert ws(8, 8, 70, 70, 300, 59, 512, 512) - ws(8, 8, 70, 70, 300, 59, 512, 256) == 8 * 512 * 256 * 8


def test_python_surface():
    from zeroshotsemanticsegmentation_amd import datasets, engine, heads, synthetic_dataset, trainer_fcn
    sig = inspect.signature(heads.pseudo)
    assert list(sig.parameters) == ["stride", "fmap", "emb", "H", "W", "target", "unseen", "gamma", "keep", "conf_floor", "cand_label",
                                    "want"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["gamma"], d["keep"], d["conf_floor"], d["cand_label"], d["want"]) == (0.0, 0.3, -2.0, datasets.HIDDEN_LABEL, ())
    assert datasets.HIDDEN_LABEL == -3
    assert inspect.signature(engine.TrainStep.__init__).parameters["pseudo"].default is None
    assert callable(engine.TrainStep.set_pseudo_active)
    assert "nothing is exchanged" in " ".join(engine.TrainStep.__init__.__doc__.split())          # the DDP note
    params = inspect.signature(trainer_fcn.Trainer.__init__).parameters
    assert params["pseudo"].default is None and params["pseudo_start_epoch"].default == 0
    for cls in (datasets.PascalContext, datasets.PascalVOC, synthetic_dataset.SyntheticSegmentation):
        assert inspect.signature(cls.__init__).parameters["hide_unseen"].default is False
    # heads.pseudo_permille: keep rounded to permille, (0, 1] only
    from zeroshotsemanticsegmentation_amd._lib import SznError
    assert heads.pseudo_permille(0.3) == 300 and heads.pseudo_permille(1) == 1000 and heads.pseudo_permille(0.0004) == 1
    assert heads.pseudo_permille(0.2996) == 300 and heads.pseudo_permille(0.001) == 1
    for bad in (0, 0.0, -0.1, 1.0001, 2, float("nan"), float("inf"), None, "x"):
        with pytest.raises(SznError):
            heads.pseudo_permille(bad)


def test_heads_pseudo_refuses_on_the_host():
    import torch
    from zeroshotsemanticsegmentation_amd import heads
    from zeroshotsemanticsegmentation_amd._lib import SznError
    fmap, emb = torch.zeros(1, 2, 2, 24), torch.zeros(21, 20)
    tgt = torch.full((1, 33, 47), -3, dtype=torch.int64)
    ok = dict(gamma=0.0, keep=0.3, conf_floor=0.2)
    for kw in (dict(ok, keep=0), dict(ok, keep=1.5), dict(ok, keep=float("nan")), dict(ok, gamma=float("nan")),
               dict(ok, conf_floor=float("inf")), dict(ok, cand_label=0), dict(ok, cand_label=3), dict(ok, want=("nope",))):
        with pytest.raises(SznError):
            heads.pseudo(32, fmap, emb, 33, 47, tgt, [2, 5], **kw)
    with pytest.raises(SznError):
        heads.pseudo(32, fmap.double(), emb, 33, 47, tgt, [2, 5])
    with pytest.raises(SznError):
        heads.pseudo(32, fmap, emb, 33, 47, None, [2, 5])
    with pytest.raises(SznError):
        heads.pseudo(32, fmap, emb, 33, 47, tgt[:, :5], [2, 5])


def test_train_step_refuses_on_the_host():
    import numpy as np
    from zeroshotsemanticsegmentation_amd import engine, models
    from zeroshotsemanticsegmentation_amd._lib import SznError
    emb = np.zeros((21, 20), dtype=np.float32)
    m = models.FCN32s(20)

    def msg(**kw):
        with pytest.raises(SznError) as e:
            engine.TrainStep(m, embeddings=kw.pop("embeddings", emb), **kw)
        return str(e.value)
    ok = dict(unseen=[2, 5], gamma=0.0, keep=0.3, conf_floor=0.2)
    assert "pseudo" in msg(embeddings=None, loss="cross_entropy", pseudo=ok)
    assert "pseudo" in msg(pseudo=dict(ok, unseen=[]))
    assert "pseudo" in msg(pseudo=dict(ok, keep=0.0)) and "pseudo" in msg(pseudo=dict(ok, keep=1.5))
    assert "finite" in msg(pseudo=dict(ok, gamma=float("nan"))) and "finite" in msg(pseudo=dict(ok, conf_floor=float("inf")))
    assert "pseudo" in msg(pseudo=dict(ok, top=3)) and "pseudo" in msg(pseudo=[2, 5])
    # a well-formed request gets as far as the device check
    for loss in ("cos", "mse", "sim_ce"):
        assert "GPU" in msg(loss=loss, pseudo=ok)
    assert engine.TrainStep._check_pseudo(dict(unseen=[5, 2, 5]), "cos") == ([2, 5], 0.0, 300, -2.0)


def test_parser_flags_and_refused_combinations():
    from zeroshotsemanticsegmentation_amd import train, trainer_fcn
    P = train.build_parser()
    args = P.parse_args(['-c', '18', '--pseudo-label', '0.3', '--pseudo-gamma', '0.125', '--pseudo-floor', '0.2', '--pseudo-start-epoch', '2'])
    assert (args.pseudo_label, args.pseudo_gamma, args.pseudo_floor, args.pseudo_start_epoch, args.hide_unseen) == (0.3, 0.125, 0.2, 2, False)
    none = P.parse_args(['-c', '18'])
    assert none.pseudo_label is None and none.pseudo_gamma is None and none.pseudo_floor is None and none.pseudo_start_epoch is None
    assert none.hide_unseen is False and P.parse_args(['-c', '18', '--hide-unseen']).hide_unseen is True
    cfg = train.update_cfg_with_args(train.configurations[18], args)
    assert cfg['train_unseen'] or cfg['val_unseen']
    train.check_pseudo(0.3, 0.125, 0.2, 2, False, cfg)
    train.check_pseudo(1.0, None, None, None, True, cfg)
    train.check_pseudo(None, None, None, None, False, dict(cfg, fcn_loss='cross_entropy', embed_dim=0))     # nothing asked: nothing refused
    train.check_pseudo(None, None, None, None, True, cfg)
    for keep in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(Exception):
            train.check_pseudo(keep, None, None, None, False, cfg)
    for kw in (dict(gamma=float("nan")), dict(floor=float("inf")), dict(start_epoch=-1)):
        with pytest.raises(Exception):
            train.check_pseudo(0.3, kw.get("gamma"), kw.get("floor"), kw.get("start_epoch"), False, cfg)
    for sat in ((0.1, None, None), (None, 0.2, None), (None, None, 1)):                                     # satellites without --pseudo-label
        with pytest.raises(Exception):
            train.check_pseudo(None, sat[0], sat[1], sat[2], False, cfg)
    for bad in (dict(cfg, train_unseen=[], val_unseen=[]), dict(cfg, fcn_loss='cross_entropy', embed_dim=0)):
        with pytest.raises(Exception):
            train.check_pseudo(0.3, None, None, None, False, bad)
    with pytest.raises(Exception):
        train.check_pseudo(None, None, None, None, True, dict(cfg, train_unseen=[], val_unseen=[]))       # --hide-unseen with nothing to hide
    # the rule both layers share, case by case
    ok = dict(has_unseen=True, embed_cfg=True, n_class=33)
    assert trainer_fcn.pseudo_refused(**ok) is None
    for key, val in (("has_unseen", False), ("embed_cfg", False), ("n_class", 257)):
        assert isinstance(trainer_fcn.pseudo_refused(**dict(ok, **{key: val})), str), key
