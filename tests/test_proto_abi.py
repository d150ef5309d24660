"""CPU: the class-prototype entry points (szn_class_proto, szn_class_proto_workspace_bytes) are declared in include/szn.h, exported by
libszn_hip.so and bound in _lib.SIGNATURES with the header's parameter lists; bad arguments are refused on the host before anything
touches a device; the Python surface (heads.class_proto, FCN32s.class_prototypes, utils.blend_prototypes, datasets.SupportSet,
Trainer(proto=, support_loader=), train.py flags) carries the new names, and the configurations that cannot adapt raise."""
import ctypes
import inspect
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW = {"szn_class_proto": "int", "szn_class_proto_workspace_bytes": "size_t"}


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
    assert param.startswith("int "), param
    return "int"


def test_signatures_match_header():
    from zeroshotsemanticsegmentation_amd import _lib as L
    kinds = {L._I: "int", L._P: "ptr", L._CS: "class_set"}
    for name, res in NEW.items():
        got_res, args = L.SIGNATURES[name]
        assert got_res is (L._I if res == "int" else L._SZ), name
        assert [kinds[a] for a in args] == [_kind(p) for p in _header_params(name, res)], name
    names = [p.split()[-1].lstrip("*") for p in _header_params("szn_class_proto", "int")]
    assert names == ["stride", "B", "h", "w", "E", "ldc", "c0", "H", "W", "crop", "K", "coarse", "labels", "classes", "mode", "accumulate",
                     "sums", "counts", "workspace", "stream"]
    assert [p.split()[-1] for p in _header_params("szn_class_proto_workspace_bytes", "size_t")] == ["stride", "B", "h", "w", "E", "K"]
    assert re.search(r"#define\s+SZN_PROTO_RAW\s+0\b", _header()) and L.PROTO_RAW == 0
    assert re.search(r"#define\s+SZN_PROTO_UNIT\s+1\b", _header()) and L.PROTO_UNIT == 1
    full = open(os.path.join(ROOT, "include", "szn.h")).read()
    assert "szn_last_kernel(): proto_finalize_kernel; szn_prev_kernel(): proto_reduce_kernel" in full


def test_library_exports_the_entry_points_and_refuses_bad_arguments():
    import __graft_entry__ as g
    from zeroshotsemanticsegmentation_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        g.build()
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
    lib = L.load()
    assert lib.szn_version() >= 112
    # refused on the host, before anything touches a device (the buffers only stand for non-NULL, 16-byte aligned pointers)
    raw = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p((ctypes.addressof(raw) + 15) & ~15)
    ALL = object()

    def call(stride=32, K=21, classes=ALL, mode=1, acc=0, coarse=p, labels=p, sums=p, counts=p, ws=p, crop=19, ldc=24, c0=0, h=2, w=2, E=20,
             B=1, H=33, W=47):
        cs = None if classes is ALL else classes
        return lib.szn_class_proto(stride, B, h, w, E, ldc, c0, H, W, crop, K, coarse, labels, cs, mode, acc, sums, counts, ws, None)
    assert call(stride=16) == -1 and call(stride=0) == -1
    assert call(B=0) == -1 and call(h=0) == -1 and call(w=-1) == -1 and call(E=0) == -1 and call(K=0) == -1 and call(H=0) == -1 and call(W=0) == -1
    assert call(K=257) == -1 and b"SZN_MAX_CLASSES" in lib.szn_last_error()
    assert call(ldc=19) == -1 and call(c0=5) == -1 and call(c0=-1) == -1            # ldc < c0 + E
    assert call(w=1) == -1 and b"crop window" in lib.szn_last_error()              # 47 + 19 > 32 * (1 + 1)
    assert call(crop=64) == -1 and call(crop=-1) == -1
    for name in ("coarse", "labels", "sums", "counts", "ws"):
        assert call(**{name: None}) == -1 and b"required" in lib.szn_last_error(), name
    assert call(ws=ctypes.c_void_p(p.value + 4)) == -1 and b"aligned" in lib.szn_last_error()
    assert call(classes=L.class_set([21])) == -1 and call(K=70, classes=L.class_set([70])) == -1 and b">= K" in lib.szn_last_error()
    empty = L.ClassSet()
    assert call(classes=ctypes.byref(empty)) == -1 and b"empty" in lib.szn_last_error()
    assert call(mode=2) == -1 and call(mode=-1) == -1 and b"mode" in lib.szn_last_error()
    assert call(acc=2) == -1 and call(acc=-1) == -1 and b"accumulate" in lib.szn_last_error()
    assert call(E=20000, ldc=20000) == -3 and b"LDS" in lib.szn_last_error()        # E too large for LDS: unsupported
    ws = lib.szn_class_proto_workspace_bytes
    assert ws(32, 1, 2, 2, 20, 21) > 0 and ws(8, 2, 14, 14, 300, 59) > 0
    assert ws(16, 1, 2, 2, 20, 21) == 0 and ws(32, 1, 2, 2, 20, 257) == 0 and ws(32, 0, 2, 2, 20, 21) == 0 and ws(32, 1, 2, 0, 20, 21) == 0
    assert ws(32, 1, 0, 2, 20, 21) == 0 and ws(32, 1, 2, 2, 0, 21) == 0 and ws(32, 1, 2, 2, 20, 0) == 0 and ws(32, 1, 2, 2, 20000, 21) == 0
    # nothing grows with the image: the Gram table (8 floats per position), the per-cell [4][K] and per-position [K] double tables, at
    # most 64 [K][E] partial sums, the [K][2] counts
    B, h, w, E, K = 8, 70, 70, 300, 59
    own = B * h * w * 8 * 4 + K * 2 * 8 + B * (h + 1) * (w + 1) * 4 * K * 8 + B * h * w * K * 8 + 64 * K * E * 8
    assert own <= ws(8, B, h, w, E, K) <= own + 5 * 256
    assert ws(8, B, h, w, E, K) < B * 512 * 512 * E * 4 // 8                         # an eighth of the (B,E,H,W) score


def test_python_surface():
    from zeroshotsemanticsegmentation_amd import datasets, heads, models, trainer_fcn, utils
    sig = inspect.signature(heads.class_proto)
    assert list(sig.parameters)[:9] == ["stride", "fmap", "H", "W", "labels", "K", "classes", "mode", "out"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["classes"], d["mode"], d["out"]) == (None, "unit", None)
    assert callable(heads.proto_call) and callable(heads.proto_workspace_bytes)
    assert heads.proto_mode("unit") == 1 and heads.proto_mode("raw") == 0
    for cls in (models.FCN32s, models.FCN8s):
        sig = inspect.signature(cls.class_prototypes)
        assert list(sig.parameters) == ["self", "x", "labels", "K", "classes", "mode", "out"]
        assert sig.parameters["mode"].default == "unit" and sig.parameters["classes"].default is None and sig.parameters["out"].default is None
    assert models.FCN8s.class_prototypes is models.FCN32s.class_prototypes                    # inherited: stride 8 through _head_map
    sig = inspect.signature(utils.blend_prototypes)
    assert list(sig.parameters) == ["embeddings", "sums", "counts", "classes", "alpha", "min_pixels"] and sig.parameters["min_pixels"].default == 1
    assert list(inspect.signature(datasets.SupportSet.__init__).parameters) == ["self", "base", "classes", "shots"]
    assert callable(datasets._SegmentationDataset.class_presence)
    p = inspect.signature(trainer_fcn.Trainer.__init__).parameters
    assert p["proto"].default is None and p["support_loader"].default is None
    assert list(p)[-4:] == ["calibration", "calib_sweep", "eval_scales", "eval_flip"]       # the pinned tail stays
    assert list(inspect.signature(trainer_fcn.proto_refused).parameters) == ["has_unseen", "embed_cfg", "n_class", "shots"]
    assert callable(trainer_fcn.Trainer.adapted_embeddings) and callable(trainer_fcn.Trainer.pool_prototypes)
    assert trainer_fcn.PROTO_ALPHA == 0.5


def test_heads_class_proto_refuses_on_the_host():
    import torch
    from zeroshotsemanticsegmentation_amd import heads
    from zeroshotsemanticsegmentation_amd._lib import SznError
    fmap = torch.zeros(1, 2, 2, 24)
    lbl = torch.zeros((1, 33, 47), dtype=torch.int64)
    for kw in (dict(mode="mean"), dict(mode=1), dict(classes=[]), dict(classes=[21]), dict(classes=[-1]), dict(E=0), dict(E=25),
               dict(out=(torch.zeros(21, 24), torch.zeros(21, 2, dtype=torch.int64))),                       # float32 sums
               dict(out=(torch.zeros(21, 20, dtype=torch.float64), torch.zeros(21, 2, dtype=torch.int64)))):  # E mismatch (24 channels)
        with pytest.raises(SznError):
            heads.class_proto(32, fmap, 33, 47, lbl, 21, **kw)
    for K in (0, 257):
        with pytest.raises(SznError):
            heads.class_proto(32, fmap, 33, 47, lbl, K)
    with pytest.raises(SznError):
        heads.class_proto(32, fmap.double(), 33, 47, lbl, 21)
    with pytest.raises(SznError):
        heads.class_proto(32, fmap, 33, 47, None, 21)
    with pytest.raises(SznError):
        heads.class_proto(32, fmap, 33, 47, lbl[:, :5], 21)
    with pytest.raises(SznError):
        heads.class_proto(16, fmap, 33, 47, lbl, 21)                                  # bad geometry: workspace bytes 0


def test_parser_flags_and_refused_combinations():
    from zeroshotsemanticsegmentation_amd import train, trainer_fcn
    P = train.build_parser()
    args = P.parse_args(['-c', '18', '--proto-shots', '5', '--proto-alpha', '0.25', '--proto-mode', 'raw', '--proto-min-pixels', '9'])
    assert (args.proto_shots, args.proto_alpha, args.proto_mode, args.proto_min_pixels) == (5, 0.25, 'raw', 9)
    none = P.parse_args(['-c', '18'])
    assert none.proto_shots is None and none.proto_alpha is None and none.proto_mode is None and none.proto_min_pixels is None
    with pytest.raises(SystemExit):
        P.parse_args(['-c', '18', '--proto-shots', '5', '--proto-mode', 'mean'])
    helptext = " ".join(P.format_help().split())
    assert "N has no default" in helptext and "default 0.5: the midpoint" in helptext and "nobody has tuned" in helptext
    cfg = train.update_cfg_with_args(train.configurations[18], args)
    assert cfg['embed_dim'] and cfg['fcn_loss'] in ("cos", "mse", "sim_ce", "rank") and (cfg['train_unseen'] or cfg['val_unseen'])
    assert train.check_proto(5, 0.25, 'raw', 9, cfg) == dict(shots=5, alpha=0.25, mode='raw', min_pixels=9)
    assert train.check_proto(1, None, None, None, cfg) == dict(shots=1, alpha=0.5, mode='unit', min_pixels=1)      # the defaults
    assert train.check_proto(None, None, None, None, dict(cfg, fcn_loss='cross_entropy', embed_dim=0)) is None     # nothing asked
    for shots in (0, -3):
        with pytest.raises(Exception):
            train.check_proto(shots, None, None, None, cfg)
    for kw in (dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=float("nan")), dict(min_pixels=0)):
        with pytest.raises(Exception):
            train.check_proto(5, kw.get("alpha"), None, kw.get("min_pixels"), cfg)
    for sat in ((0.5, None, None), (None, 'raw', None), (None, None, 3)):                                          # satellites alone
        with pytest.raises(Exception):
            train.check_proto(None, *sat, cfg)
    with pytest.raises(Exception):
        train.check_proto(5, None, None, None, dict(cfg, fcn_loss='cross_entropy', embed_dim=0))
    with pytest.raises(Exception):
        train.check_proto(5, None, None, None, dict(cfg, train_unseen=[], val_unseen=[]))
    # the rule both layers share, case by case
    assert trainer_fcn.proto_refused(True, True, 33, 5) is None
    assert "embedding" in trainer_fcn.proto_refused(True, False, 33, 5)
    assert "unseen" in trainer_fcn.proto_refused(False, True, 33, 5)
    assert "shots" in trainer_fcn.proto_refused(True, True, 33, 0) and "shots" in trainer_fcn.proto_refused(True, True, 33, 1.5)
    assert "256" in trainer_fcn.proto_refused(True, True, 257, 5)


def test_trainer_refuses_on_the_host(tmp_path):
    import numpy as np
    import torch
    from zeroshotsemanticsegmentation_amd import models, trainer_fcn
    from zeroshotsemanticsegmentation_amd._lib import SznError
    from zeroshotsemanticsegmentation_amd.datasets import SupportSet
    from zeroshotsemanticsegmentation_amd.synthetic_dataset import SyntheticSegmentation
    ds = SyntheticSegmentation(split='train', n_images=2, size=(32, 40), n_class=21, embed_dim=20, unseen=[], seed=3)
    loader = torch.utils.data.DataLoader(ds, batch_size=1)
    support = torch.utils.data.DataLoader(SupportSet(ds, [2, 5], 1), batch_size=1)
    emb = np.load(os.path.join(ROOT, "tests", "golden", "embeddings_pascal_20.npy"))[:21]

    def msg(**kw):
        args = dict(cuda=True, model=models.FCN32s(20), optimizer=None, train_loader=loader, val_loader=loader, log_dir=str(tmp_path / "log"),
                    dataset='pascal', max_epoch=1, tb_writer=None, pixel_embeddings=20, loss_func='cos', unseen=[2, 5], val_unseen=[5],
                    embed_arr=emb, proto=dict(shots=1), support_loader=support)
        args.update(kw)
        with pytest.raises(SznError) as e:
            trainer_fcn.Trainer(**args)
        return str(e.value)
    assert "embedding" in msg(pixel_embeddings=None, loss_func='cross_entropy')
    assert "unseen classes" in msg(unseen=[], val_unseen=[])
    assert "shots" in msg(proto=dict(shots=0)) and "shots" in msg(proto=dict(alpha=0.5))
    assert "alpha" in msg(proto=dict(shots=1, alpha=2.0)) and "min_pixels" in msg(proto=dict(shots=1, min_pixels=0))
    assert "mode" in msg(proto=dict(shots=1, mode="mean")) and "proto" in msg(proto=dict(shots=1, top=3))
    assert "support_loader" in msg(support_loader=None) and "support_loader" in msg(proto=None)
    # a well-formed request builds (on the host: nothing runs before validate()) and writes the log header
    t = trainer_fcn.Trainer(cuda=True, model=models.FCN32s(20), optimizer=None, train_loader=loader, val_loader=loader,
                            log_dir=str(tmp_path / "log"), dataset='pascal', max_epoch=1, tb_writer=None, pixel_embeddings=20,
                            loss_func='cos', unseen=[2, 5], val_unseen=[5], embed_arr=emb, proto=dict(shots=1), support_loader=support)
    assert t.proto == dict(shots=1, alpha=0.5, mode="unit", min_pixels=1)
    assert open(str(tmp_path / "log" / "proto_log.csv")).read() == 'epoch,class,name,shots,participating,contributing,cos_word_proto\n'
