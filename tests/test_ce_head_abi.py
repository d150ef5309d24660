"""CPU: the fused softmax cross-entropy head (szn_fused_ce_head) is declared in include/szn.h, exported by libszn_hip.so and bound
in _lib.SIGNATURES with the header's parameter list; TrainStep accepts the cross-entropy loss and both models have
softmax_predict (no compute calls)."""
import ctypes
import inspect
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW = ("szn_fused_ce_head_workspace_bytes", "szn_fused_ce_head")


def _header_params(name):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "szn.h")).read(), flags=re.S)
    m = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
    assert m, name
    return [p.strip() for p in m.group(1).split(",")]


def _ctype_of(param):
    if "*" in param or param.startswith("szn_stream_t"):
        return "ptr"
    assert param.startswith("int "), param
    return "int"


def test_header_declares_ce_head():
    names = [p.split()[-1].lstrip("*") for p in _header_params("szn_fused_ce_head")]
    assert names == ["stride", "B", "h", "w", "C", "ldc", "c0", "H", "W", "crop", "coarse", "target", "weight", "size_average",
                     "loss", "stats", "pred", "dcoarse_dtype", "dcoarse", "workspace", "stream"]
    assert [p.split()[-1] for p in _header_params("szn_fused_ce_head_workspace_bytes")] == ["stride", "B", "h", "w", "C"]


def test_signatures_match_header():
    from zeroshotsemanticsegmentation_amd import _lib as L
    kinds = {L._I: "int", L._P: "ptr"}
    res, args = L.SIGNATURES["szn_fused_ce_head"]
    assert res is L._I
    assert [kinds[a] for a in args] == [_ctype_of(p) for p in _header_params("szn_fused_ce_head")]
    res, args = L.SIGNATURES["szn_fused_ce_head_workspace_bytes"]
    assert res is L._SZ and args == [L._I] * 5


def test_library_exports_ce_head():
    import __graft_entry__ as g
    from zeroshotsemanticsegmentation_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        g.build()
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
    loaded = L.load()
    assert loaded.szn_version() >= 103
    # bad arguments are refused on the host, before anything touches a device
    assert loaded.szn_fused_ce_head_workspace_bytes(32, 2, 17, 17, 21) > 0
    assert loaded.szn_fused_ce_head_workspace_bytes(16, 2, 17, 17, 21) == 0
    assert loaded.szn_fused_ce_head_workspace_bytes(32, 2, 17, 17, 257) == 0
    ws = ctypes.create_string_buffer(16)
    common = (None, None, 0, None, None, None, L.SZN_F32, None)     # target .. dcoarse
    assert loaded.szn_fused_ce_head(16, 1, 4, 4, 21, 64, 0, 64, 64, 19, ws, *common, ws, None) == -3          # stride
    assert loaded.szn_fused_ce_head(32, 1, 4, 4, 257, 320, 0, 64, 64, 19, ws, *common, ws, None) == -3       # C > 256
    assert loaded.szn_fused_ce_head(32, 1, 4, 4, 21, 64, 0, 150, 64, 19, ws, *common, ws, None) == -1        # crop window
    assert loaded.szn_fused_ce_head(32, 1, 4, 4, 21, 16, 0, 64, 64, 19, ws, *common, ws, None) == -1         # ldc < c0 + C
    assert loaded.szn_fused_ce_head(32, 1, 4, 4, 21, 64, 0, 64, 64, 19, ws, *common, ws, None) == -1         # pred-only, no pred


def test_train_step_accepts_cross_entropy():
    from zeroshotsemanticsegmentation_amd import engine
    sig = inspect.signature(engine.TrainStep.__init__)
    assert sig.parameters["embeddings"].default is None
    assert sig.parameters["class_weight"].default is None and sig.parameters["size_average"].default is False
    src = inspect.getsource(engine.TrainStep.__init__)
    assert '"cross_entropy"' in src


def test_softmax_predict_on_both_models():
    from zeroshotsemanticsegmentation_amd import models
    for cls in (models.FCN32s, models.FCN8s):
        assert callable(getattr(cls, "softmax_predict", None)), cls
        assert list(inspect.signature(cls.softmax_predict).parameters) == ["self", "x", "target", "weight"]
    assert models.FCN8s.softmax_predict is not models.FCN32s.softmax_predict


def test_trainer_routes_softmax_config():
    from zeroshotsemanticsegmentation_amd import trainer_fcn
    assert hasattr(trainer_fcn.Trainer, "_ce_cfg")
