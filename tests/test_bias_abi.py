"""CPU: the fused sim_ce head with the unseen-bias term (szn_fused_simce_bias_head / _prepared) is declared in include/szn.h with
szn_fused_simce_head's argument list plus (bias_unseen, weight, hidden_label) behind `temperature`, exported by libszn_hip.so and bound
in _lib.SIGNATURES; the header states the definition; its own argument errors are refused on the host; heads, TrainStep, the trainer and
train.py accept the bias loss with sim_ce alone (no compute calls)."""
import ctypes
import inspect
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW = ("szn_fused_simce_bias_head", "szn_fused_simce_bias_head_prepared")


def _header():
    return open(os.path.join(ROOT, "include", "szn.h")).read()


def _header_params(name):
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
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
    if param.startswith("int64_t "):
        return "int64"
    assert param.startswith("int "), param
    return "int"


def test_header_declares_the_documented_argument_order():
    sce = _header_params("szn_fused_simce_head")
    at = sce.index("float temperature") + 1
    want = sce[:at] + ["const szn_class_set* bias_unseen", "float weight", "int64_t hidden_label"] + sce[at:]
    for name in NEW:
        assert _header_params(name) == want, name
    assert _header_params("szn_fused_simce_head_prepared") == sce


def test_header_states_the_definition():
    txt = " ".join(_header().split())
    m = re.search(r"/\* ---- fused sim_ce head with the unseen-bias term.*?\*/ int szn_fused_simce_bias_head\(", txt)
    assert m
    doc = m.group(0)
    for phrase in ("lambda * -log sum_{u in U} p_u", "logsumexp_{all k} z_k - logsumexp_{u in U} z_u", "ALL K classes",
                   "own maximum", "q_k = 1[k in U] exp(z_k - m_U)", "N_b = labelled + hidden px", "one joint mean per image",
                   "hidden_label >= -1", "bit for bit"):
        assert phrase in doc, phrase


def test_signatures_match_header():
    from zeroshotsemanticsegmentation_amd import _lib as L
    kinds = {L._I: "int", L._P: "ptr", L._CS: "class_set", L._F: "float", L._I64: "int64"}
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
    assert loaded.szn_version() >= 111
    # refused on the host, before anything touches a device (the buffer only stands for non-NULL, 16-B aligned pointers)
    raw = ctypes.create_string_buffer(64)
    ws = ctypes.c_void_p((ctypes.addressof(raw) + 15) & ~15)
    K = 21
    head = (32, 1, 4, 4, 20, 64, 0, 64, 64, 19, K, ws, ws, None, None, 0, None)               # stride .. group_map: a pred-only call
    tail = (None, None, ws, L.SZN_F32, None, ws, None)                                          # loss .. stream
    U = L.class_set([2, 5])
    for name in NEW:
        fn = getattr(loaded, name)
        for uns in (None, L.class_set(range(K))):                                               # empty, all
            assert fn(*head, None, 0.1, uns, 1.0, -3, *tail) == -1, name
            assert "bias set" in loaded.szn_last_error().decode()
        assert fn(*head, None, 0.1, L.class_set([K]), 1.0, -3, *tail) == -1 and "bias set" in loaded.szn_last_error().decode()
        for weight in (0.0, -1.0, float("nan"), float("inf")):
            assert fn(*head, None, 0.1, U, weight, -3, *tail) == -1, (name, weight)
            assert "weight" in loaded.szn_last_error().decode()
        for hl in (-1, 0, 5):
            assert fn(*head, None, 0.1, U, 1.0, hl, *tail) == -1, (name, hl)
            assert "hidden label" in loaded.szn_last_error().decode()
        # what sim_ce refuses
        for T in (0.0, -1.0, float("nan"), float("inf")):
            assert fn(*head, None, T, U, 1.0, -3, *tail) == -1 and "temperature" in loaded.szn_last_error().decode()
        assert fn(*head, L.class_set([K]), 0.1, U, 1.0, -3, *tail) == -1 and "exclude" in loaded.szn_last_error().decode()
        assert fn(*head, L.class_set(range(K)), 0.1, U, 1.0, -3, *tail) == -1 and "competing" in loaded.szn_last_error().decode()
        # the MSE head's checks carry over
        assert fn(16, *head[1:], None, 0.1, U, 1.0, -3, *tail) == -3, name                      # stride
        assert fn(*head[:10], 257, *head[11:], None, 0.1, U, 1.0, -3, *tail) == -3, name        # K > 256
        assert fn(*head[:7], 150, *head[8:], None, 0.1, U, 1.0, -3, *tail) == -1, name          # crop window
        assert fn(*head, None, 0.1, U, 1.0, -3, None, None, ws, L.SZN_F32, ws, ws, None) == -1, name      # dcoarse without target
        assert fn(*head[:4], 9000, 9100, *head[6:], None, 0.1, U, 1.0, -3, *tail) == -3, name   # LDS budget


def test_python_surface_takes_the_bias_term():
    from zeroshotsemanticsegmentation_amd import _lib as L, datasets, engine, heads, trainer_fcn, utils
    assert callable(heads.sim_ce_bias) and callable(utils.sim_ce_bias_loss)
    for fn in (heads.embed, heads.embed_predict, heads.embed_loss):
        assert inspect.signature(fn).parameters["bias"].default is None
    p = inspect.signature(utils.sim_ce_bias_loss).parameters
    assert list(p) == ["score", "target", "embed", "exclude", "temperature", "unseen", "weight", "hidden_label"]
    assert p["hidden_label"].default == datasets.HIDDEN_LABEL
    assert heads.bias_args("sim_ce", None, 21) == () and heads.bias_args("cos", None, 21) == ()
    cs, weight, hidden = heads.bias_args("sim_ce", dict(unseen=[2, 5], weight=0.5), 21)
    assert cs is not None and weight == 0.5 and hidden == datasets.HIDDEN_LABEL
    assert heads.bias_args("sim_ce", dict(unseen=[2], weight=2, hidden=-5), 21)[2] == -5
    for kind in ("cos", "mse", "rank"):
        with pytest.raises(L.SznError) as ei:
            heads.bias_args(kind, dict(unseen=[2], weight=1.0), 21)
        assert "sim_ce" in str(ei.value)
    for bad in (dict(unseen=[], weight=1.0), dict(unseen=range(21), weight=1.0), dict(unseen=[21], weight=1.0),
                dict(unseen=[-1], weight=1.0), dict(unseen=[2], weight=0.0), dict(unseen=[2], weight=float("nan")),
                dict(unseen=[2], weight=float("inf")), dict(unseen=[2], weight=1.0, hidden=-1), dict(unseen=[2]),
                dict(weight=1.0), dict(unseen=[2], weight=1.0, share=0.1), dict(unseen=[2], weight="much")):
        with pytest.raises(L.SznError):
            heads.bias_args("sim_ce", bad, 21)
    params = inspect.signature(engine.TrainStep.__init__).parameters
    assert params["bias"].default is None and callable(engine.TrainStep.set_bias_active)
    params = inspect.signature(trainer_fcn.Trainer.__init__).parameters
    assert params["bias_loss"].default is None and params["bias_start_epoch"].default == 0
    assert trainer_fcn.bias_refused(True, 20, "sim_ce", 21) is None
    assert "sim_ce" in trainer_fcn.bias_refused(True, 20, "cos", 21)
    assert "sim_ce" in trainer_fcn.bias_refused(True, 0, "sim_ce", 21)
    assert "unseen classes" in trainer_fcn.bias_refused(False, 20, "sim_ce", 21)
    assert "256" in trainer_fcn.bias_refused(True, 20, "sim_ce", 300)


def test_train_step_checks_the_bias_term_before_any_device_work():
    import numpy as np
    from zeroshotsemanticsegmentation_amd import _lib as L, engine, models
    m = models.FCN32s(20)
    emb = np.load(os.path.join(ROOT, "tests", "golden", "embeddings_context_20.npy"))
    ok = dict(unseen=[2, 5, 8], weight=0.5)
    with pytest.raises(L.SznError) as ei:                # past every host check: the next refusal is the device's (CPU model here)
        engine.TrainStep(m, emb, loss="sim_ce", sim_exclude=[2, 5, 8], bias=ok)
    assert "GPU" in str(ei.value)
    for loss in ("cos", "mse", "rank"):
        with pytest.raises(L.SznError) as ei:
            engine.TrainStep(m, emb, loss=loss, bias=ok)
        assert "bias loss belongs to loss 'sim_ce'" in str(ei.value)
    with pytest.raises(L.SznError) as ei:
        engine.TrainStep(m, None, loss="cross_entropy", bias=ok)
    assert "sim_ce" in str(ei.value)
    with pytest.raises(L.SznError) as ei:
        engine.TrainStep(m, emb, loss="sim_ce", fused_head=False, bias=ok)
    assert "fused head only" in str(ei.value)
    for bad, word in ((dict(unseen=[], weight=0.5), "unseen"), (dict(unseen=range(len(emb)), weight=0.5), "unseen"),
                      (dict(unseen=[len(emb)], weight=0.5), "unseen"), (dict(unseen=[2], weight=0.0), "weight"),
                      (dict(unseen=[2], weight=float("nan")), "weight"), (dict(unseen=[2], weight=1.0, hidden=-1), "hidden"),
                      ([2, 5], "dict")):
        with pytest.raises(L.SznError) as ei:
            engine.TrainStep(m, emb, loss="sim_ce", bias=bad)
        assert word in str(ei.value) and "GPU" not in str(ei.value), (bad, str(ei.value))


def test_cli_flags():
    from zeroshotsemanticsegmentation_amd import train
    from zeroshotsemanticsegmentation_amd.configs import configurations
    p = train.build_parser()
    args = p.parse_args(['-c', '18', '-loss', 'sim_ce', '--bias-loss', '0.5', '--bias-start-epoch', '2', '--precision', 'fp16'])
    cfg = train.update_cfg_with_args(configurations[args.config], args)
    train.validate_cfg(cfg)
    assert cfg['fcn_loss'] == 'sim_ce' and args.bias_loss == 0.5 and args.bias_start_epoch == 2
    train.check_bias(args.bias_loss, args.bias_start_epoch, cfg)
    train.check_precision(args.precision, cfg)
    plain = p.parse_args(['-c', '18', '-loss', 'sim_ce'])
    assert plain.bias_loss is None and plain.bias_start_epoch is None           # no default for lambda: off
    train.check_bias(None, None, cfg)
    help_text = " ".join(p.format_help().split())
    assert "--bias-loss" in help_text and "--bias-start-epoch" in help_text and "implies --hide-unseen" in help_text
    for loss in ('cos', 'mse', 'rank'):
        other = train.update_cfg_with_args(configurations[18], p.parse_args(['-c', '18', '-loss', loss]))
        with pytest.raises(Exception) as ei:
            train.check_bias(0.5, None, other)
        assert "--bias-loss needs -loss sim_ce" in str(ei.value)
    with pytest.raises(Exception) as ei:
        train.check_bias(None, 1, cfg)
    assert "--bias-start-epoch needs --bias-loss" in str(ei.value)
    for bad in (0.0, -0.5, float("inf"), float("nan")):
        with pytest.raises(Exception) as ei:
            train.check_bias(bad, None, cfg)
        assert "LAMBDA" in str(ei.value)
    with pytest.raises(Exception):
        train.check_bias(0.5, -1, cfg)
    with pytest.raises(Exception) as ei:
        train.check_bias(0.5, None, dict(cfg, train_unseen=[], val_unseen=[]))
    assert "unseen classes" in str(ei.value)
