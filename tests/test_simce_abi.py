"""CPU: the fused similarity cross-entropy head (szn_fused_simce_head / _prepared) is declared in include/szn.h with the MSE head's
argument list plus `exclude` and `temperature` before `loss`, exported by libszn_hip.so and bound in _lib.SIGNATURES; its own
argument errors are refused on the host; heads, TrainStep, the models, the trainer and train.py accept the sim_ce loss (no compute calls)."""
import ctypes
import inspect
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW = ("szn_fused_simce_head", "szn_fused_simce_head_prepared")


def _header_params(name):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "szn.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
    assert m, name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def _ctype_of(param):
    if "szn_class_set" in param:
        return "class_set"
    if "*" in param or param.startswith("szn_stream_t"):
        return "ptr"
    if param.startswith("float "):
        return "float"
    assert param.startswith("int "), param
    return "int"


def test_header_declares_the_documented_argument_order():
    mse = _header_params("szn_fused_mse_head")
    at = mse.index("float* loss")
    want = mse[:at] + ["const szn_class_set* exclude", "float temperature"] + mse[at:]
    for name in NEW:
        assert _header_params(name) == want, name


def test_signatures_match_header():
    from zeroshotsemanticsegmentation_amd import _lib as L
    kinds = {L._I: "int", L._P: "ptr", L._CS: "class_set", L._F: "float"}
    for name in NEW:
        res, args = L.SIGNATURES[name]
        assert res is L._I
        assert [kinds[a] for a in args] == [_ctype_of(p) for p in _header_params(name)], name


def test_library_exports_the_head_and_refuses_bad_arguments():
    import __graft_entry__ as g
    from zeroshotsemanticsegmentation_amd import _lib as L
    if not os.path.exists(L.LIB_PATH) or not hasattr(ctypes.CDLL(L.LIB_PATH), NEW[0]):
        g.build()
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
    loaded = L.load()
    # refused on the host, before anything touches a device (the buffer only stands for non-NULL, 16-B aligned pointers)
    raw = ctypes.create_string_buffer(64)
    ws = ctypes.c_void_p((ctypes.addressof(raw) + 15) & ~15)
    head = (32, 1, 4, 4, 20, 64, 0, 64, 64, 19, 21, ws, ws, None, None, 0, None)              # stride .. group_map: a pred-only call
    tail = (None, None, ws, L.SZN_F32, None, ws, None)                                          # loss .. stream
    for name in NEW:
        fn = getattr(loaded, name)
        for temp in (0.0, -0.5, float("nan"), float("inf")):
            assert fn(*head, None, temp, *tail) == -1, (name, temp)
            assert "temperature" in loaded.szn_last_error().decode()
        assert fn(*head, L.class_set([21]), 0.1, *tail) == -1 and "exclude" in loaded.szn_last_error().decode()      # a class >= K
        assert fn(*head, L.class_set(range(21)), 0.1, *tail) == -1 and "competing" in loaded.szn_last_error().decode()
        # the MSE head's checks carry over
        assert fn(16, *head[1:], None, 0.1, *tail) == -3, name                                   # stride
        assert fn(*head[:10], 257, *head[11:], None, 0.1, *tail) == -3, name                     # K > 256
        assert fn(*head[:7], 150, *head[8:], None, 0.1, *tail) == -1, name                       # crop window
        assert fn(*head, None, 0.1, None, None, ws, L.SZN_F32, ws, ws, None) == -1, name         # dcoarse without target


def test_python_surface_takes_sim_ce():
    from zeroshotsemanticsegmentation_amd import _lib as L, engine, heads, models, train, trainer_fcn, utils
    assert heads.embed_kind("sim_ce") == "sim_ce"
    assert callable(heads.sim_ce) and callable(heads.sim_ce_predict) and callable(utils.sim_ce_loss)
    for fn in (heads.embed, heads.embed_predict):
        params = inspect.signature(fn).parameters
        assert params["exclude"].default is None and params["temperature"].default is None
    with pytest.raises(L.SznError):                      # the two arguments belong to sim_ce alone (checked before any call)
        heads._sim_args("cos", [1], None)
    with pytest.raises(L.SznError):
        heads._sim_args("mse", None, 0.1)
    assert heads._sim_args("cos", None, None) == ()
    cs, temp = heads._sim_args("sim_ce", None, None)
    assert cs is None and temp == heads.SIM_TEMPERATURE == 0.1
    params = inspect.signature(engine.TrainStep.__init__).parameters
    assert params["sim_exclude"].default is None and params["sim_temperature"].default is None
    for cls in (models.FCN32s, models.FCN8s):
        assert list(inspect.signature(cls.szn_predict_sim_ce).parameters) == list(inspect.signature(cls.szn_predict).parameters)
        m = cls.__new__(cls)
        assert cls._sim_kw(m, "cos") == {} and cls._sim_kw(m, "sim_ce") == dict(exclude=None, temperature=None)
    t = object.__new__(trainer_fcn.Trainer)
    t.pixel_embeddings, t.loss_func = 20, "sim_ce"
    assert t._embed_cfg() is True
    assert "sim_temperature" in inspect.signature(trainer_fcn.Trainer.__init__).parameters


def test_train_step_accepts_sim_ce_on_the_fused_head_only():
    import numpy as np
    from zeroshotsemanticsegmentation_amd import _lib as L, engine, models
    m = models.FCN32s(20)
    emb = np.load(os.path.join(ROOT, "tests", "golden", "embeddings_context_20.npy"))
    with pytest.raises(L.SznError) as ei:                # past the loss check: the next refusal is the device's (CPU model here)
        engine.TrainStep(m, emb, loss="sim_ce", sim_exclude=[1, 2], sim_temperature=0.1)
    assert "GPU" in str(ei.value)
    with pytest.raises(L.SznError) as ei:
        engine.TrainStep(m, emb, loss="sim_ce", fused_head=False)
    assert "fused head only" in str(ei.value)
    with pytest.raises(L.SznError) as ei:
        engine.TrainStep(m, emb, loss="cos", sim_temperature=0.1)
    assert "sim_ce" in str(ei.value)


def test_cli_flags():
    from zeroshotsemanticsegmentation_amd import train
    from zeroshotsemanticsegmentation_amd.configs import configurations
    p = train.build_parser()
    args = p.parse_args(['-c', '18', '-loss', 'sim_ce', '--sim-temperature', '0.1', '--precision', 'fp16'])
    cfg = train.update_cfg_with_args(configurations[args.config], args)
    train.validate_cfg(cfg)
    assert cfg['fcn_loss'] == 'sim_ce' and args.sim_temperature == 0.1
    train.check_sim_temperature(args.sim_temperature, cfg)
    train.check_precision(args.precision, cfg)                                  # fp16 is accepted: the fused step scales the loss
    train.check_eval_views([0.5, 1.0], True, cfg)
    assert p.parse_args(['-c', '18', '-loss', 'sim_ce']).sim_temperature is None        # the default is heads.SIM_TEMPERATURE
    help_text = p.format_help()
    assert "not a tuned value" in " ".join(help_text.split())
    other = train.update_cfg_with_args(configurations[18], p.parse_args(['-c', '18', '--sim-temperature', '0.1']))
    if other['fcn_loss'] != 'sim_ce':
        with pytest.raises(Exception) as ei:
            train.check_sim_temperature(0.1, other)
        assert "--sim-temperature needs -loss sim_ce" in str(ei.value)
    with pytest.raises(Exception):
        train.check_sim_temperature(0.0, cfg)
    with pytest.raises(Exception) as ei:                                        # no embedding: the rule that covers cos and mse
        train.validate_cfg(dict(cfg, embed_dim=0))
    assert "pixel embedding dimensionality" in str(ei.value)
