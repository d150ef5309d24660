"""CPU: the fused hinge ranking head (szn_fused_rank_head / _prepared) is declared in include/szn.h with the MSE head's argument list plus
`exclude`, `margin` and `hardest` before `loss`, exported by libszn_hip.so and bound in _lib.SIGNATURES; its own argument errors are
refused on the host; heads, TrainStep, the models, the trainer and train.py accept the rank loss (no compute calls)."""
import ctypes
import inspect
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW = ("szn_fused_rank_head", "szn_fused_rank_head_prepared")


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
    want = mse[:at] + ["const szn_class_set* exclude", "float margin", "int hardest"] + mse[at:]
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
    assert loaded.szn_version() >= 110
    # refused on the host, before anything touches a device (the buffer only stands for non-NULL, 16-B aligned pointers)
    raw = ctypes.create_string_buffer(64)
    ws = ctypes.c_void_p((ctypes.addressof(raw) + 15) & ~15)
    head = (32, 1, 4, 4, 20, 64, 0, 64, 64, 19, 21, ws, ws, None, None, 0, None)              # stride .. group_map: a pred-only call
    tail = (None, None, ws, L.SZN_F32, None, ws, None)                                          # loss .. stream
    for name in NEW:
        fn = getattr(loaded, name)
        for margin in (-0.5, -1e-9, float("nan"), float("inf"), float("-inf")):
            assert fn(*head, None, margin, 0, *tail) == -1, (name, margin)
            assert "margin" in loaded.szn_last_error().decode()
        for hardest in (-1, 2, 7):
            assert fn(*head, None, 0.1, hardest, *tail) == -1, (name, hardest)
            assert "hardest" in loaded.szn_last_error().decode()
        assert fn(*head, L.class_set([21]), 0.1, 0, *tail) == -1 and "exclude" in loaded.szn_last_error().decode()      # a class >= K
        for excl in (range(21), range(20), range(1, 21)):                                        # none, or one class left
            assert fn(*head, L.class_set(excl), 0.1, 1, *tail) == -1 and "competing" in loaded.szn_last_error().decode()
        # the MSE head's checks carry over
        assert fn(16, *head[1:], None, 0.1, 0, *tail) == -3, name                                # stride
        assert fn(*head[:10], 257, *head[11:], None, 0.1, 0, *tail) == -3, name                  # K > 256
        assert fn(*head[:7], 150, *head[8:], None, 0.1, 0, *tail) == -1, name                    # crop window
        assert fn(*head, None, 0.1, 0, None, None, ws, L.SZN_F32, ws, ws, None) == -1, name      # dcoarse without target
        assert fn(*head[:4], 9000, 9100, *head[6:], None, 0.1, 0, *tail) == -3, name             # LDS budget
        assert "LDS" in loaded.szn_last_error().decode()


def test_python_surface_takes_rank():
    from zeroshotsemanticsegmentation_amd import _lib as L, engine, heads, models, trainer_fcn, utils
    assert heads.embed_kind("rank") == "rank"
    with pytest.raises(L.SznError) as ei:
        heads.embed_kind("hinge")
    assert "loss must be" in str(ei.value)
    assert callable(heads.rank) and callable(heads.rank_predict) and callable(utils.rank_loss)
    assert heads.RANK_MARGIN == 0.1
    for fn in (heads.embed, heads.embed_predict, heads.embed_loss):
        params = inspect.signature(fn).parameters
        assert list(params)[-2:] == ["margin", "hardest"] and params["margin"].default is None and params["hardest"].default is None
        assert params["exclude"].default is None
    p = inspect.signature(utils.rank_loss).parameters
    assert list(p) == ["score", "target", "embed", "exclude", "margin", "hardest"]
    assert p["exclude"].default is None and p["margin"].default == 0.1 and p["hardest"].default is False
    for kind in ("cos", "mse", "sim_ce"):                  # the two arguments belong to rank alone (checked before any call)
        with pytest.raises(L.SznError):
            heads._rank_args(kind, None, 0.1, None)
        with pytest.raises(L.SznError):
            heads._rank_args(kind, None, None, True)
        assert heads._rank_args(kind, None, None, None) == ()
    with pytest.raises(L.SznError):                        # and sim_ce's temperature is none of rank's
        heads._loss_args("rank", None, 0.1, None, None)
    with pytest.raises(L.SznError):
        heads._loss_args("cos", None, None, 0.2, None)
    cs, margin, hardest = heads._rank_args("rank", None, None, None)
    assert cs is None and margin == heads.RANK_MARGIN and hardest == 0
    cs, margin, hardest = heads._rank_args("rank", [1, 2], 0.25, True)
    assert cs is not None and margin == 0.25 and hardest == 1
    params = inspect.signature(engine.TrainStep.__init__).parameters
    assert params["rank_margin"].default is None and params["rank_hardest"].default is False
    for cls in (models.FCN32s, models.FCN8s):
        assert list(inspect.signature(cls.szn_predict_rank).parameters) == list(inspect.signature(cls.szn_predict).parameters)
        m = cls.__new__(cls)
        assert cls._head_kw(m, "cos") == {} and cls._head_kw(m, "sim_ce") == cls._sim_kw(m, "sim_ce")
        assert cls._head_kw(m, "rank") == dict(exclude=None, margin=None, hardest=False)
        p = inspect.signature(cls.set_rank).parameters
        assert [p[k].default for k in ("exclude", "margin", "hardest")] == [None, None, False]
    t = object.__new__(trainer_fcn.Trainer)
    t.pixel_embeddings, t.loss_func = 20, "rank"
    assert t._embed_cfg() is True
    params = inspect.signature(trainer_fcn.Trainer.__init__).parameters
    assert params["rank_margin"].default is None and params["rank_hardest"].default is False


def test_train_step_accepts_rank_on_the_fused_head_only():
    import numpy as np
    from zeroshotsemanticsegmentation_amd import _lib as L, engine, models
    m = models.FCN32s(20)
    emb = np.load(os.path.join(ROOT, "tests", "golden", "embeddings_context_20.npy"))
    with pytest.raises(L.SznError) as ei:                # past the loss check: the next refusal is the device's (CPU model here)
        engine.TrainStep(m, emb, loss="rank", sim_exclude=[1, 2], rank_margin=0.2, rank_hardest=True)
    assert "GPU" in str(ei.value)
    with pytest.raises(L.SznError) as ei:
        engine.TrainStep(m, emb, loss="rank", fused_head=False)
    assert "fused head only" in str(ei.value)
    with pytest.raises(L.SznError) as ei:
        engine.TrainStep(m, emb, loss="cos", rank_margin=0.1)
    assert "rank" in str(ei.value)
    with pytest.raises(L.SznError) as ei:
        engine.TrainStep(m, emb, loss="sim_ce", rank_hardest=True)
    assert "rank" in str(ei.value)
    with pytest.raises(L.SznError) as ei:
        engine.TrainStep(m, emb, loss="rank", sim_temperature=0.1)
    assert "sim_ce" in str(ei.value)


def test_cli_flags():
    from zeroshotsemanticsegmentation_amd import train
    from zeroshotsemanticsegmentation_amd.configs import configurations
    p = train.build_parser()
    args = p.parse_args(['-c', '18', '-loss', 'rank', '--rank-margin', '0.2', '--rank-hardest', '--precision', 'fp16'])
    cfg = train.update_cfg_with_args(configurations[args.config], args)
    train.validate_cfg(cfg)
    assert cfg['fcn_loss'] == 'rank' and args.rank_margin == 0.2 and args.rank_hardest is True
    train.check_rank(args.rank_margin, args.rank_hardest, cfg)
    train.check_precision(args.precision, cfg)                                  # fp16 is accepted: the fused step scales the loss
    train.check_eval_views([0.5, 1.0], True, cfg)
    plain = p.parse_args(['-c', '18', '-loss', 'rank'])
    assert plain.rank_margin is None and plain.rank_hardest is False            # the default is heads.RANK_MARGIN
    train.check_rank(None, False, cfg)
    train.check_rank(0.0, False, cfg)
    help_text = " ".join(p.format_help().split())
    assert "--rank-margin" in help_text and "--rank-hardest" in help_text and "DeViSE" in help_text
    assert help_text.count("not a tuned value") >= 2                            # --sim-temperature's and --rank-margin's
    other = train.update_cfg_with_args(configurations[18], p.parse_args(['-c', '18', '-loss', 'cos']))
    for margin, hardest in ((0.1, False), (None, True)):
        with pytest.raises(Exception) as ei:
            train.check_rank(margin, hardest, other)
        assert "need -loss rank" in str(ei.value)
    for bad in (-0.1, float("inf"), float("nan")):
        with pytest.raises(Exception):
            train.check_rank(bad, False, cfg)
    with pytest.raises(Exception) as ei:                                        # no embedding: the rule that covers every embedding loss
        train.validate_cfg(dict(cfg, embed_dim=0))
    assert "pixel embedding dimensionality" in str(ei.value)
    with pytest.raises(Exception) as ei:                                        # the refusal still names the losses it does accept
        train.check_precision('fp16', dict(cfg, fcn_loss='cross_entropy', embed_dim=20))
    assert "'mse'" in str(ei.value) and "'rank'" in str(ei.value)
