"""CPU: the multi-scale inference entry points (szn_resize_flip_f32, szn_ms_head, szn_ms_head_workspace_bytes) and szn_ms_view_t are
declared in include/szn.h, exported by libszn_hip.so and bound in _lib.SIGNATURES with the header's parameter lists; the struct layout
matches; bad arguments are refused on the host before anything touches a device; the Python surface carries the new keywords."""
import ctypes
import inspect
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW = {"szn_resize_flip_f32": "int", "szn_ms_head": "int", "szn_ms_head_workspace_bytes": "size_t"}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "szn.h")).read(), flags=re.S)


def _header_params(name, res):
    m = re.search(r"\b%s\s+%s\s*\(([^)]*)\)\s*;" % (res, name), _header())
    assert m, name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def _kind(param):
    if "szn_class_set" in param:
        return "class_set"
    if "szn_ms_view_t" in param:
        return "views"
    if "*" in param or param.startswith("szn_stream_t"):
        return "ptr"
    assert param.startswith("int "), param
    return "int"


def test_signatures_match_header():
    from zeroshotsemanticsegmentation_amd import _lib as L
    kinds = {L._I: "int", L._P: "ptr", L._CS: "class_set", L._MV: "views"}
    for name, res in NEW.items():
        got_res, args = L.SIGNATURES[name]
        assert got_res is (L._I if res == "int" else L._SZ), name
        assert [kinds[a] for a in args] == [_kind(p) for p in _header_params(name, res)], name
    names = [p.split()[-1].lstrip("*") for p in _header_params("szn_ms_head", "int")]
    assert names == ["stride", "B", "E", "K", "H", "W", "crop", "n_views", "views", "embed", "unseen", "group_mode", "group_map",
                     "target", "pred", "acc", "workspace", "stream"]


def test_view_struct_layout_matches_header():
    from zeroshotsemanticsegmentation_amd import _lib as L
    m = re.search(r"typedef struct szn_ms_view\s*\{(.*?)\}\s*szn_ms_view_t;", _header(), flags=re.S)
    assert m
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype = ctypes.c_void_p if "*" in decl else ctypes.c_int
        assert "*" in decl or decl.startswith("int "), decl
        for n in decl.replace("const float*", "").replace("int ", "").split(","):
            fields.append((n.strip(), ctype))
    assert [(n, t) for n, t in L.MsView._fields_] == fields
    assert fields[0][0] == "coarse" and [n for n, _ in fields[1:]] == ["h", "w", "ldc", "c0", "Hs", "Ws", "flip"]
    assert ctypes.sizeof(L.MsView) == 40 and L.MsView.h.offset == 8 and L.MsView.flip.offset == 32
    assert re.search(r"#define\s+SZN_MS_MAX_VIEWS\s+16\b", _header()) and L.MS_MAX_VIEWS == 16


def test_library_exports_the_entry_points_and_refuses_bad_arguments():
    import __graft_entry__ as g
    from zeroshotsemanticsegmentation_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        g.build()
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
    lib = L.load()
    assert lib.szn_version() >= 105
    # refused on the host, before anything touches a device (the buffer only stands for non-NULL, 16-byte aligned pointers)
    raw = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p((ctypes.addressof(raw) + 15) & ~15)

    def views(n=2, **over):
        arr = (L.MsView * max(n, 1))()
        for rec in arr:
            rec.coarse, rec.h, rec.w, rec.ldc, rec.c0, rec.Hs, rec.Ws, rec.flip = p.value, 2, 2, 24, 0, 33, 47, 0
            for k, v in over.items():
                setattr(rec, k, v)
        return arr

    def head(stride=32, K=21, n=2, arr=None, embed=p, unseen=None, mode=0, gmap=None, target=None, pred=p, crop=19):
        return lib.szn_ms_head(stride, 1, 20, K, 33, 47, crop, n, arr if arr is not None else views(n), embed, unseen, mode, gmap,
                               target, pred, None, p, None)
    assert head(n=0) == -1 and head(n=L.MS_MAX_VIEWS + 1, arr=views(L.MS_MAX_VIEWS + 1)) == -1
    assert head(stride=16) == -1 and head(stride=0) == -1
    assert head(arr=views(coarse=None)) == -1 and b"coarse" in lib.szn_last_error()
    assert head(embed=None) == -1 and head(pred=None) == -1
    assert head(arr=views(Hs=0)) == -1 and head(arr=views(Ws=0)) == -1
    assert head(arr=views(h=1, Hs=50)) == -1                     # 50 + 19 > 32 * (1 + 1): the map cannot cover the view
    assert head(arr=views(w=2, Ws=78)) == -1                     # 78 + 19 > 32 * (2 + 1)
    assert head(K=257) == -1
    assert head(mode=1) == -1 and head(mode=2) == -1 and head(mode=3) == -1
    assert head(unseen=L.class_set([21])) == -1 and head(K=70, unseen=L.class_set([70])) == -1
    assert head(arr=views(ldc=19)) == -1
    assert head(arr=views(h=32768)) == -1 and head(arr=views(w=40000)) == -1      # h * w is an int in the kernels
    assert lib.szn_ms_head_workspace_bytes(32, 1, 20, 21, 2, views(h=32768)) == 0
    ws = lib.szn_ms_head_workspace_bytes
    assert ws(32, 1, 20, 21, 2, views()) > 0 and ws(8, 2, 300, 59, 2, views(ldc=300)) > ws(8, 1, 300, 59, 2, views(ldc=300))
    assert ws(16, 1, 20, 21, 2, views()) == 0 and ws(32, 1, 20, 21, 0, views()) == 0 and ws(32, 1, 20, 257, 2, views()) == 0
    assert ws(32, 1, 20, 21, 2, views(Hs=0)) == 0
    rf = lib.szn_resize_flip_f32
    assert rf(1, 33, 47, None, 17, 24, 0, p, None) == -1 and rf(1, 33, 47, p, 17, 24, 0, None, None) == -1
    assert rf(1, 33, 47, p, 0, 24, 0, p, None) == -1 and rf(0, 33, 47, p, 17, 24, 0, p, None) == -1


def test_python_surface_takes_the_new_keywords():
    from zeroshotsemanticsegmentation_amd import _lib as L, heads, models, train, trainer_fcn
    for cls in (models.FCN32s, models.FCN8s):
        sig = inspect.signature(cls.ms_predict)
        assert list(sig.parameters) == ["self", "x", "embeddings", "scales", "flip", "target", "unseen", "group", "loss"]
        assert sig.parameters["flip"].default is False and sig.parameters["loss"].default == "cos"
    params = list(inspect.signature(trainer_fcn.Trainer.__init__).parameters)
    assert params[-2:] == ["eval_scales", "eval_flip"]
    assert callable(heads.ms_predict) and callable(heads.resize_flip)
    assert heads.ms_views(33, 47, (1.5, 0.5, 1), True) == [(17, 24, False), (17, 24, True), (33, 47, False), (33, 47, True),
                                                           (50, 71, False), (50, 71, True)]
    assert heads.ms_views(1, 1, (0.25, 1.0)) == [(1, 1, False), (1, 1, False)]
    with pytest.raises(L.SznError):
        heads.ms_views(33, 47, (0.5, 1.5))
    args = train.build_parser().parse_args(['-c', '18', '--eval-scales', '0.5', '1', '--eval-flip'])
    assert args.eval_scales == [0.5, 1.0] and args.eval_flip is True
    cfg = train.update_cfg_with_args(train.configurations[18], args)
    train.check_eval_views(args.eval_scales, args.eval_flip, cfg)
    with pytest.raises(Exception):
        train.check_eval_views([0.5, 2.0], False, cfg)
    with pytest.raises(Exception):
        train.check_eval_views([1.0], True, dict(cfg, fcn_loss='cross_entropy', embed_dim=0))
    none = train.build_parser().parse_args(['-c', '18'])
    assert none.eval_scales is None and none.eval_flip is False
