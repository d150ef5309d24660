"""CPU: the grouped fused head (szn_fused_head_grouped / _prepared) is declared in include/szn.h, exported by libszn_hip.so and
bound in _lib.SIGNATURES with the header's parameter list; the public Python entry points exist (no compute calls)."""
import ctypes
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW = ("szn_fused_head_grouped", "szn_fused_head_grouped_prepared")


def _header_params(name):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "szn.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
    assert m, name
    return [p.strip() for p in m.group(1).split(",")]


def _ctype_of(param):
    if "*" in param:
        return "class_set" if "szn_class_set" in param else "ptr"
    if param.startswith("szn_stream_t"):
        return "ptr"
    assert param.startswith("int "), param
    return "int"


def test_header_declares_grouped_head():
    for name in NEW:
        params = _header_params(name)
        names = [p.split()[-1].lstrip("*") for p in params]
        assert names[:11] == ["stride", "B", "h", "w", "E", "ldc", "c0", "H", "W", "crop", "K"]
        for must in ("unseen", "group_mode", "group_map", "target", "pred", "loss", "stats", "dcoarse", "workspace", "stream"):
            assert must in names, (name, must)
    assert _header_params(NEW[0]) == [p for p in _header_params(NEW[1])]


def test_signatures_match_header():
    from zeroshotsemanticsegmentation_amd import _lib as L
    kinds = {L._I: "int", L._P: "ptr", L._CS: "class_set"}
    for name in NEW:
        res, args = L.SIGNATURES[name]
        assert res is L._I
        assert [kinds[a] for a in args] == [_ctype_of(p) for p in _header_params(name)], name


def test_library_exports_grouped_head():
    import __graft_entry__ as g
    from zeroshotsemanticsegmentation_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        g.build()
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
    assert L.load().szn_version() >= 101


def test_public_entry_points():
    import inspect
    from zeroshotsemanticsegmentation_amd import engine, models
    for cls in (models.FCN32s, models.FCN8s):
        sig = inspect.signature(cls.szn_predict)
        assert list(sig.parameters) == ["self", "x", "embeddings", "unseen", "target", "group"]
        assert sig.parameters["group"].default == "seenmask" and sig.parameters["target"].default is None
    assert inspect.signature(engine.TrainStep).parameters["forced_unseen"].default is None
