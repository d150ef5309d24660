"""CPU: the hard-pixel-mining entry points (szn_ohem_head, szn_ohem_head_workspace_bytes) are declared in include/szn.h, exported by
libszn_hip.so and bound in _lib.SIGNATURES with the header's parameter lists; bad arguments are refused on the host before anything
touches a device; the Python surface (heads.ohem, TrainStep(ohem=), Trainer(ohem=, ohem_start_epoch=), train.py flags) carries the new
names, and the configurations that cannot mine raise."""
import ctypes
import inspect
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW = {"szn_ohem_head": "int", "szn_ohem_head_workspace_bytes": "size_t"}


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
    names = [p.split()[-1].lstrip("*") for p in _header_params("szn_ohem_head", "int")]
    assert names == ["stride", "B", "h", "w", "E", "ldc", "c0", "H", "W", "crop", "K", "coarse", "embed", "target", "skip", "keep_permille",
                     "thresh", "drop_label", "target_out", "conf", "qhist", "cut", "counts", "workspace", "stream"]
    assert [p.split()[-1] for p in _header_params("szn_ohem_head_workspace_bytes", "size_t")] == ["stride", "B", "h", "w", "E", "K", "H",
                                                                                                "W"]
    assert re.search(r"#define\s+SZN_OHEM_BINS\s+1024\b", _header()) and L.OHEM_BINS == 1024


def test_library_exports_the_entry_points_and_refuses_bad_arguments():
    import __graft_entry__ as g
    from zeroshotsemanticsegmentation_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        g.build()
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
    lib = L.load()
    assert lib.szn_version() >= 108
    # refused on the host, before anything touches a device (the buffers only stand for non-NULL, 16-byte aligned pointers)
    raw, raw2 = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
    p = ctypes.c_void_p((ctypes.addressof(raw) + 15) & ~15)
    q = ctypes.c_void_p((ctypes.addressof(raw2) + 15) & ~15)

    def head(stride=32, K=21, keep=250, thresh=0.0, label=-1, skip=(), coarse=p, embed=p, target=p, out=q, ws=p, crop=19, ldc=24, h=2,
             w=2, E=20):
        return lib.szn_ohem_head(stride, 1, h, w, E, ldc, 0, 33, 47, crop, K, coarse, embed, target, L.class_set(skip), keep, thresh,
                                 label, out, None, None, None, None, ws, None)
    # what szn_pseudo_head refuses about the shared arguments
    assert head(stride=16) == -1 and head(stride=0) == -1
    assert head(coarse=None) == -1 and head(embed=None) == -1 and head(ws=None) == -1
    assert head(K=257) == -1 and head(K=0) == -1
    assert head(ldc=19) == -1                                   # ldc < c0 + E
    assert head(w=1) == -1                                      # 47 + 19 > 32 * (1 + 1): the map cannot cover the image
    assert head(crop=64) == -1 and head(h=0) == -1
    assert head(ws=ctypes.c_void_p(p.value + 4)) == -1          # workspace not 16-byte aligned
    assert head(E=20000, ldc=20000) == -3                       # E too large for LDS: unsupported, as there
    # its own
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert head(thresh=bad) == -1 and b"finite" in lib.szn_last_error()
    assert head(keep=0) == -1 and head(keep=1001) == -1 and head(keep=-1) == -1 and b"keep_permille" in lib.szn_last_error()
    assert head(label=0) == -1 and head(label=7) == -1 and b"drop_label" in lib.szn_last_error()
    assert head(skip=(21,)) == -1 and head(K=70, skip=(70,)) == -1 and b"skip" in lib.szn_last_error()
    assert head(K=3, skip=(0, 1, 2)) == -1 and b"every class" in lib.szn_last_error()
    assert head(target=None) == -1 and head(out=None) == -1
    assert head(out=p) == -1 and b"alias" in lib.szn_last_error()
    ws = lib.szn_ohem_head_workspace_bytes
    assert ws(32, 1, 2, 2, 20, 21, 33, 47) > 0
    assert ws(16, 1, 2, 2, 20, 21, 33, 47) == 0 and ws(32, 1, 2, 2, 20, 257, 33, 47) == 0 and ws(32, 0, 2, 2, 20, 21, 33, 47) == 0
    assert ws(32, 1, 2, 0, 20, 21, 33, 47) == 0 and ws(32, 1, 2, 2, 20, 21, 0, 47) == 0 and ws(32, 1, 2, 2, 20, 21, 33, 0) == 0
    # the fused head's workspace + the [B][1024] table + cuts + 4 bytes per pixel
    base = lib.szn_fused_head_workspace_bytes(8, 70, 70, 300, 59)
    own = 8 * 1024 * 8 + 8 * 4 + 8 * 512 * 512 * 4
    assert base + own <= ws(8, 8, 70, 70, 300, 59, 512, 512) <= base + own + 1024
    assert ws(8, 8, 70, 70, 300, 59, 512, 512) - ws(8, 8, 70, 70, 300, 59, 512, 256) == 8 * 512 * 256 * 4


def test_python_surface():
    from zeroshotsemanticsegmentation_amd import engine, heads, trainer_fcn
    from zeroshotsemanticsegmentation_amd._lib import SznError
    sig = inspect.signature(heads.ohem)
    assert list(sig.parameters) == ["stride", "fmap", "emb", "H", "W", "target", "keep", "thresh", "skip", "drop_label", "want"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert d["keep"] is inspect.Parameter.empty
    assert (d["thresh"], d["skip"], d["drop_label"], d["want"]) == (None, None, heads.OHEM_DROP_LABEL, ())
    assert heads.OHEM_DROP_LABEL == -1
    assert "counts" in inspect.signature(heads.ohem_call).parameters and callable(heads.ohem_workspace_bytes)
    assert inspect.signature(engine.TrainStep.__init__).parameters["ohem"].default is None
    assert callable(engine.TrainStep.set_ohem_active)
    doc = " ".join(engine.TrainStep.__init__.__doc__.split())
    assert "each rank's own images: nothing is exchanged" in doc                                  # the DDP note
    params = list(inspect.signature(trainer_fcn.Trainer.__init__).parameters)
    i = params.index("ohem")
    assert params[i - 1:i + 3] == ["pseudo_start_epoch", "ohem", "ohem_start_epoch", "calibration"]
    assert params[-4:] == ["calibration", "calib_sweep", "eval_scales", "eval_flip"]
    p = inspect.signature(trainer_fcn.Trainer.__init__).parameters
    assert p["ohem"].default is None and p["ohem_start_epoch"].default == 0
    # heads.ohem_permille: keep rounded to permille, (0, 1] only
    assert heads.ohem_permille(0.25) == 250 and heads.ohem_permille(1) == 1000 and heads.ohem_permille(0.0004) == 1
    assert heads.ohem_permille(0.2496) == 250 and heads.ohem_permille(0.001) == 1
    for bad in (0, 0.0, -0.1, 1.0001, 2, float("nan"), float("inf"), None, "x"):
        with pytest.raises(SznError):
            heads.ohem_permille(bad)


def test_heads_ohem_refuses_on_the_host():
    import torch
    from zeroshotsemanticsegmentation_amd import heads
    from zeroshotsemanticsegmentation_amd._lib import SznError
    fmap, emb = torch.zeros(1, 2, 2, 24), torch.zeros(21, 20)
    tgt = torch.zeros((1, 33, 47), dtype=torch.int64)
    for kw in (dict(keep=0), dict(keep=1.5), dict(keep=float("nan")), dict(keep=0.25, thresh=float("nan")),
               dict(keep=0.25, thresh=float("inf")), dict(keep=0.25, drop_label=0), dict(keep=0.25, drop_label=3),
               dict(keep=0.25, want=("nope",)), dict(keep=0.25, skip=[21]), dict(keep=0.25, skip=[-1]),
               dict(keep=0.25, skip=list(range(21)))):
        with pytest.raises(SznError):
            heads.ohem(32, fmap, emb, 33, 47, tgt, **kw)
    with pytest.raises(SznError):
        heads.ohem(32, fmap.double(), emb, 33, 47, tgt, 0.25)
    with pytest.raises(SznError):
        heads.ohem(32, fmap, emb, 33, 47, None, 0.25)
    with pytest.raises(SznError):
        heads.ohem(32, fmap, emb, 33, 47, tgt[:, :5], 0.25)


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
    ok = dict(keep=0.25, thresh=0.0)
    assert "ohem" in msg(embeddings=None, loss="cross_entropy", ohem=ok)
    assert "ohem" in msg(ohem=dict(ok, keep=0.0)) and "ohem" in msg(ohem=dict(ok, keep=1.5)) and "ohem" in msg(ohem=dict(thresh=0.0))
    assert "finite" in msg(ohem=dict(ok, thresh=float("nan"))) and "finite" in msg(ohem=dict(ok, thresh=float("-inf")))
    assert "ohem" in msg(ohem=dict(ok, top=3)) and "ohem" in msg(ohem=0.25) and "ohem" in msg(ohem=dict(ok, thresh="x"))
    # a well-formed request gets as far as the device check
    for loss in ("cos", "mse", "sim_ce"):
        assert "GPU" in msg(loss=loss, ohem=ok)
        assert "GPU" in msg(loss=loss, ohem=dict(keep=1.0))
    assert engine.TrainStep._check_ohem(dict(keep=0.25), "cos") == (250, -2.0)
    assert engine.TrainStep._check_ohem(dict(keep=1, thresh=0.5), "sim_ce") == (1000, 0.5)
    assert engine.TrainStep._check_ohem(dict(keep=0.25, thresh=None), "mse") == (250, -2.0)


def test_parser_flags_and_refused_combinations():
    from zeroshotsemanticsegmentation_amd import train, trainer_fcn
    P = train.build_parser()
    args = P.parse_args(['-c', '18', '--ohem', '0.25', '--ohem-thresh', '0.5', '--ohem-start-epoch', '2'])
    assert (args.ohem, args.ohem_thresh, args.ohem_start_epoch) == (0.25, 0.5, 2)
    none = P.parse_args(['-c', '18'])
    assert none.ohem is None and none.ohem_thresh is None and none.ohem_start_epoch is None
    helptext = " ".join(P.format_help().split())
    assert "KEEP has no default" in helptext and "nobody has tuned" in helptext
    cfg = train.update_cfg_with_args(train.configurations[18], args)
    assert cfg['embed_dim'] and cfg['fcn_loss'] in ("cos", "mse", "sim_ce")
    train.check_ohem(0.25, 0.5, 2, cfg)
    train.check_ohem(1.0, None, None, cfg)
    train.check_ohem(0.25, -3.0, 0, dict(cfg, train_unseen=[], val_unseen=[]))                 # no unseen classes needed
    train.check_ohem(None, None, None, dict(cfg, fcn_loss='cross_entropy', embed_dim=0))      # nothing asked: nothing refused
    for keep in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(Exception):
            train.check_ohem(keep, None, None, cfg)
    for kw in (dict(thresh=float("nan")), dict(thresh=float("inf")), dict(start_epoch=-1)):
        with pytest.raises(Exception):
            train.check_ohem(0.25, kw.get("thresh"), kw.get("start_epoch"), cfg)
    for sat in ((0.2, None), (None, 1)):                                                        # satellites without --ohem
        with pytest.raises(Exception):
            train.check_ohem(None, sat[0], sat[1], cfg)
    with pytest.raises(Exception):
        train.check_ohem(0.25, None, None, dict(cfg, fcn_loss='cross_entropy', embed_dim=0))
    # the rule both layers share, case by case
    assert trainer_fcn.ohem_refused(embed_cfg=True, n_class=33) is None
    assert isinstance(trainer_fcn.ohem_refused(embed_cfg=False, n_class=33), str)
    assert isinstance(trainer_fcn.ohem_refused(embed_cfg=True, n_class=257), str)
