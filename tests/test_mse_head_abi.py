"""CPU: the fused MSE embedding head (szn_fused_mse_head / _prepared) is declared in include/szn.h, exported by libszn_hip.so and
bound in _lib.SIGNATURES with the header's parameter list; bad arguments are refused on the host; TrainStep, the models' predict
methods, the trainer and train.py's precision gate accept the mse loss (no compute calls)."""
import ctypes
import inspect
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW = ("szn_fused_mse_head", "szn_fused_mse_head_prepared")


def _header_params(name):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "szn.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
    assert m, name
    return [p.strip() for p in m.group(1).split(",")]


def _ctype_of(param):
    if "szn_class_set" in param:
        return "class_set"
    if "*" in param or param.startswith("szn_stream_t"):
        return "ptr"
    assert param.startswith("int "), param
    return "int"


def test_header_declares_mse_head_with_the_grouped_argument_list():
    want = [p.split()[-1].lstrip("*") for p in _header_params("szn_fused_head_grouped")]
    assert want[:3] == ["stride", "B", "h"] and "group_mode" in want and "unseen" in want
    for name in NEW:
        assert [p.split()[-1].lstrip("*") for p in _header_params(name)] == want, name
    assert _header_params("szn_fused_mse_head") == _header_params("szn_fused_head_grouped")


def test_signatures_match_header():
    from zeroshotsemanticsegmentation_amd import _lib as L
    kinds = {L._I: "int", L._P: "ptr", L._CS: "class_set"}
    for name in NEW:
        res, args = L.SIGNATURES[name]
        assert res is L._I
        assert [kinds[a] for a in args] == [_ctype_of(p) for p in _header_params(name)], name


def test_library_exports_mse_head_and_refuses_bad_arguments():
    import __graft_entry__ as g
    from zeroshotsemanticsegmentation_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        g.build()
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
    loaded = L.load()
    assert loaded.szn_version() >= 104
    # refused on the host, before anything touches a device (the buffer only stands for non-NULL, 16-B aligned pointers)
    raw = ctypes.create_string_buffer(64)
    ws = ctypes.c_void_p((ctypes.addressof(raw) + 15) & ~15)
    tail = (None, None, 0, None, None, None, ws, L.SZN_F32, None, ws, None)      # target .. stream: a pred-only call
    for name in NEW:
        fn = getattr(loaded, name)
        assert fn(16, 1, 4, 4, 20, 64, 0, 64, 64, 19, 21, ws, ws, *tail) == -3, name           # stride
        assert fn(32, 1, 4, 4, 20, 64, 0, 64, 64, 19, 257, ws, ws, *tail) == -3, name          # K > 256
        assert fn(32, 1, 4, 4, 20, 64, 0, 150, 64, 19, 21, ws, ws, *tail) == -1, name          # crop window
        assert fn(32, 1, 4, 4, 20, 16, 0, 64, 64, 19, 21, ws, ws, *tail) == -1, name           # ldc < c0 + E
        none_pred = tail[:6] + (None,) + tail[7:]
        assert fn(32, 1, 4, 4, 20, 64, 0, 64, 64, 19, 21, ws, ws, *none_pred[:2], 1, *none_pred[3:]) == -1, name   # mode 1, no pred
        with_dc = tail[:8] + (ws,) + tail[9:]
        assert fn(32, 1, 4, 4, 20, 64, 0, 64, 64, 19, 21, ws, ws, *with_dc) == -1, name        # dcoarse without target
        assert fn(32, 1, 4, 4, 20, 64, 0, 64, 64, 19, 21, ws, ws, *tail[:2], 2, *tail[3:]) == -1, name    # mode 2, no target


def test_train_step_accepts_mse_on_the_fused_head():
    from zeroshotsemanticsegmentation_amd import engine, heads
    assert inspect.signature(engine.TrainStep.__init__).parameters["fused_head"].default is True
    assert callable(heads.mse) and callable(heads.mse_predict)
    assert heads.embed_kind("mse") == "mse" and heads.embed_kind("cos") == "cos"
    with pytest.raises(Exception):
        heads.embed_kind("cross_entropy")
    # TrainStep(loss="mse") gets past the loss check with the fused head: the next refusal is the device's (CPU model here)
    from zeroshotsemanticsegmentation_amd import _lib as L, models
    import numpy as np
    m = models.FCN32s(20)
    emb = np.load(os.path.join(ROOT, "tests", "golden", "embeddings_context_20.npy"))
    with pytest.raises(L.SznError) as ei:
        engine.TrainStep(m, emb, loss="mse")
    assert "GPU" in str(ei.value) and "mse" not in str(ei.value)
    with pytest.raises(L.SznError) as ei:
        engine.TrainStep(m, emb, loss="l1")
    assert "loss must be" in str(ei.value)


def test_predict_methods_take_the_mse_loss():
    from zeroshotsemanticsegmentation_amd import models
    for cls in (models.FCN32s, models.FCN8s):
        sig = inspect.signature(cls.embed_predict)
        assert list(sig.parameters) == ["self", "x", "embeddings", "target", "loss"] and sig.parameters["loss"].default == "cos"
        assert list(inspect.signature(cls.szn_predict_mse).parameters) == list(inspect.signature(cls.szn_predict).parameters)
    sig = inspect.signature(models.FCN8s.embed_loss)
    assert sig.parameters["loss"].default == "cos"


def test_trainer_routes_mse_embedding_config():
    from zeroshotsemanticsegmentation_amd import trainer_fcn
    t = object.__new__(trainer_fcn.Trainer)           # the constructor needs a GPU; the routing predicate does not
    for emb, loss, want in ((20, "mse", True), (20, "cos", True), (20, "cross_entropy", False), (0, "mse", False)):
        t.pixel_embeddings, t.loss_func = emb, loss
        assert t._embed_cfg() is want, (emb, loss)


def test_cli_accepts_fp16_with_mse():
    from zeroshotsemanticsegmentation_amd import train
    from zeroshotsemanticsegmentation_amd.configs import configurations
    args = train.build_parser().parse_args(['-c', '2', '-loss', 'mse', '--precision', 'fp16'])
    cfg = train.update_cfg_with_args(configurations[args.config], args)
    train.validate_cfg(cfg)
    assert cfg['fcn_loss'] == 'mse' and cfg['embed_dim']
    train.check_precision(args.precision, cfg)                       # accepted
    bad = dict(cfg, fcn_loss='cross_entropy')                        # embedding + cross entropy: still no fused step
    with pytest.raises(Exception) as ei:
        train.check_precision('fp16', bad)
    assert "'mse'" in str(ei.value)
    train.check_precision('bf16', bad)
