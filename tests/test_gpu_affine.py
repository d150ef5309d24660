"""GPU: the affine augmentation kernel (szn_augment_affine_u8, csrc/szn_augment.hip), its Python surface (utils.augment_affine_to_device,
datasets.Augment with rotate / jitter), both trainers and the CLI against the numpy restatement of the contract in tests/helpers_affine.py.
The contract is integer-exact: every comparison of pixels is torch.equal on the float image and on the labels.

Shapes: an 11 x 15 image in a 13 x 17 canvas whose padding bytes are 255 (a tap that leaves the image shows); outputs 8 x 12 (16-byte stores)
and 7 x 10 (scalar stores, a partial last run per row); one realistic 375 x 500 -> 512 x 512 (several blocks per image)."""
import ctypes as C
import functools
import glob
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers_affine as HF  # noqa: E402
import helpers_augment as HA  # noqa: E402
from zeroshotsemanticsegmentation_amd import _lib as L  # noqa: E402
from zeroshotsemanticsegmentation_amd import datasets, engine, models, optim, train, trainer_fcn, trainer_seenmask, utils  # noqa: E402
from zeroshotsemanticsegmentation_amd.synthetic_dataset import SyntheticSegmentation  # noqa: E402

SIZE, CANVAS = (11, 15), (13, 17)
KERNELS = {(8, 12): "augment_affine_u8_kernel_v4", (7, 10): "augment_affine_u8_kernel"}
PLAIN_KERNELS = {(8, 12): "augment_u8_kernel_v4", (7, 10): "augment_u8_kernel"}
CANARY = 64
JITTER = dict(brightness=0.125, contrast=0.5, saturation=0.5, hue=18.0)


@functools.lru_cache(maxsize=None)
def batch(B=3):
    rng = np.random.RandomState(11)
    h, w = SIZE
    img = np.full((B,) + CANVAS + (3,), 255, dtype=np.uint8)
    lbl = np.full((B,) + CANVAS, 77, dtype=np.int64)
    img[:, :h, :w] = rng.randint(0, 256, (B, h, w, 3))
    lbl[:, :h, :w] = rng.randint(-1, 21, (B, h, w))
    img.setflags(write=False)
    lbl.setflags(write=False)
    return img, lbl


def launch(entry, img, lbl, rec, out_hw, canary=CANARY):
    """an augmentation entry through the C-ABI into buffers with a canary region behind each output -> (data, target, canaries untouched)"""
    B, Hm, Wm, _ = img.shape
    Ho, Wo = out_hw
    n = B * Ho * Wo
    data = torch.full((3 * n + canary,), 12345.0, device="cuda")
    target = torch.full((n + canary,), 987654321, dtype=torch.int64, device="cuda")
    mean = (C.c_double * 3)(*HA.MEAN_BGR)
    d_img, d_lbl = torch.from_numpy(np.array(img)).cuda(), torch.from_numpy(np.array(lbl)).cuda()
    d_rec = torch.from_numpy(np.asarray(rec, dtype=np.int32)).cuda()
    L.call(entry, B, Hm, Wm, L.ptr(d_img), L.ptr(d_lbl), L.ptr(d_rec), mean, Ho, Wo, L.ptr(data), L.ptr(target), L.stream_ptr())
    intact = bool((data[3 * n:] == 12345.0).all()) and bool((target[n:] == 987654321).all())
    return data[:3 * n].reshape(B, 3, Ho, Wo), target[:n].reshape(B, Ho, Wo), intact


def three_records(out_hw):
    """three different records for one launch: the bridge of a mirrored 9-word record, -33 degrees at scale 4/3 with a full colour matrix
    and the window near a corner of the bounding box (a fifth of the crop is padding, where the rotated image leaves the box's corner free),
    and a quarter turn"""
    h, w = SIZE
    full = datasets.Augment.color_words(*datasets.Augment.color_matrix(0.1, 1.3, 0.6, 25.0))
    return [HF.bridge(HA.record(h, w, 4 / 3, 1, -2, True), out_hw),
            HF.affine_words(h, w, *HF.affine_float(h, w, 4 / 3, -33.0, 3.0, 5.0, False, out_hw), color=full),
            HF.affine_words(h, w, *HF.affine_float(h, w, 1.0, 90.0))]


@pytest.mark.parametrize("out_hw", sorted(KERNELS))
def test_kernel_equals_contract(out_hw):
    img, lbl = batch()
    rec = three_records(out_hw)
    assert len({tuple(r) for r in rec}) == 3
    want_d, want_t = HF.augment(img, lbl, rec, out_hw)
    data, target, intact = launch("szn_augment_affine_u8", img, lbl, rec, out_hw)
    assert L.last_kernel() == KERNELS[out_hw]
    assert intact, "wrote behind an output"
    assert torch.equal(target.cpu(), torch.from_numpy(want_t)) and torch.equal(data.cpu(), torch.from_numpy(want_d))
    assert not (want_t == 77).any()
    pad = want_t == HF.PAD_LABEL
    assert pad[1].any() and not pad[1].all() and (want_t == -1).any()                       # the rotated image has corners to pad
    assert np.all(data.cpu().numpy().transpose(0, 2, 3, 1)[pad] == 0.0)
    # the rotated, jittered image differs from what the identity colour gives: the matrix was applied
    plain = [rec[0], rec[1][:8] + HF.IDENTITY_COLOR, rec[2]]
    assert not np.array_equal(HF.augment(img, lbl, plain, out_hw)[0][1], want_d[1])


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("out_hw", sorted(KERNELS))
def test_bridge_equals_augment_u8_on_the_device(out_hw, flip):
    img, lbl = batch()
    h, w = SIZE
    rec9 = [HA.record(h, w, s, oy, ox, flip) for s, (oy, ox) in zip((0.5, 4 / 3, 2.0), ((0, 0), (-2, -3), (3, 2)))]
    d9, t9, ok9 = launch("szn_augment_u8", img, lbl, rec9, out_hw)
    assert L.last_kernel() == PLAIN_KERNELS[out_hw]
    data, target, intact = launch("szn_augment_affine_u8", img, lbl, [HF.bridge(r, out_hw) for r in rec9], out_hw)
    assert L.last_kernel() == KERNELS[out_hw]
    assert ok9 and intact and torch.equal(target, t9) and torch.equal(data, d9)


def test_realistic_shape_with_drawn_records():
    rng = np.random.RandomState(5)
    sizes = [(375, 500), (333, 421)]
    img = rng.randint(0, 256, (2, 375, 500, 3)).astype(np.uint8)
    lbl = rng.randint(-1, 33, (2, 375, 500)).astype(np.int64)
    aug = datasets.Augment((512, 512), (0.5, 2.0), rotate=10.0, jitter=JITTER)
    rec = aug.params(sizes, 0, 1)
    assert rec.shape == (2, L.AUGA_NPARAM) and (rec[:, 3] != 0).all() and not np.array_equal(rec[0, 8:], HF.IDENTITY_COLOR)
    data, target = utils.augment_affine_to_device(img, lbl, rec, (512, 512))
    assert L.last_kernel() == "augment_affine_u8_kernel_v4"
    want_d, want_t = HF.augment(img, lbl, rec, (512, 512))
    assert torch.equal(target.cpu(), torch.from_numpy(want_t)) and torch.equal(data.cpu(), torch.from_numpy(want_d))
    # Augment.apply is the same launch
    d2, t2 = aug.apply((torch.from_numpy(img), torch.from_numpy(lbl), torch.tensor(sizes, dtype=torch.int32)), 0, 1, device="cuda")
    assert torch.equal(d2, data) and torch.equal(t2, target)
    with pytest.raises(L.SznError):
        utils.augment_affine_to_device(img, lbl, rec[:, :9].copy(), (512, 512))


def test_garbage_records_are_clamped_not_followed():
    """h > Hm, w > Wm, absurd coefficients, matrix and offset words cannot be seen from the host: the kernel clamps h, w to the canvas, the
    matrix words to +-2^20 and checks every index against the image, so the run completes and equals the contract's result under the same
    clamps (helpers_affine.fixed_point applies them)"""
    img, lbl = batch()
    big = (1 << 31) - 1
    bad = [[100, 90, big, -big, big, -big, big, -big] + [big, -big, big] * 3 + [big, -big, 12345],
           [0, -5, 65536, 0, 0, 0, 65536, 0] + [-big] * 9 + [big] * 3,
           [big, big, 30000, 70000, -100000, -70000, 30000, 400000] + [1 << 21, -(1 << 21), 1 << 19] * 3 + [-big, 0, big]]
    for out_hw in sorted(KERNELS):
        data, target, intact = launch("szn_augment_affine_u8", img, lbl, bad, out_hw)
        torch.cuda.synchronize()
        want_d, want_t = HF.augment(img, lbl, bad, out_hw)
        assert intact and torch.equal(target.cpu(), torch.from_numpy(want_t)) and torch.equal(data.cpu(), torch.from_numpy(want_d))
    assert (want_t[2] != HF.PAD_LABEL).any()                                                 # the third record does read the canvas


def test_argument_errors():
    img, lbl = batch()
    B, (Hm, Wm), (Ho, Wo) = len(img), CANVAS, (7, 10)
    t = dict(img=torch.from_numpy(np.array(img)).cuda(), lbl=torch.from_numpy(np.array(lbl)).cuda(),
             rec=torch.tensor([HF.bridge(HA.record(*SIZE, 1.0), (Ho, Wo))] * B, dtype=torch.int32, device="cuda"),
             out=torch.empty(B, 3, Ho, Wo, device="cuda"), ol=torch.empty(B, Ho, Wo, dtype=torch.int64, device="cuda"))
    mean = (C.c_double * 3)(*HA.MEAN_BGR)

    def call(B=B, Hm=Hm, Wm=Wm, Ho=Ho, Wo=Wo, mean=mean, **null):
        p = {k: (None if k in null else L.ptr(v)) for k, v in t.items()}
        L.call("szn_augment_affine_u8", B, Hm, Wm, p["img"], p["lbl"], p["rec"], mean, Ho, Wo, p["out"], p["ol"], L.stream_ptr())

    call()
    assert L.last_kernel() == "augment_affine_u8_kernel"
    L.call("szn_image_u8_to_bgr_f32", B, Hm, Wm, L.ptr(t["img"]), mean, L.ptr(torch.empty(B, 3, Hm, Wm, device="cuda")), L.stream_ptr())
    other = L.last_kernel()
    for k in t:
        with pytest.raises(L.SznError):
            call(**{k: None})
    with pytest.raises(L.SznError):
        call(mean=None)
    for kw in (dict(B=0), dict(B=-1), dict(Hm=0), dict(Wm=-3), dict(Ho=0), dict(Wo=0), dict(Wo=-4), dict(B=65536)):
        with pytest.raises(L.SznError):
            call(**kw)
    assert L.last_kernel() == other                                                          # nothing was launched
    torch.cuda.synchronize()


# ---- the trainers --------------------------------------------------------------------------------------------------------------------
E, K = 20, 33
UNSEEN, VAL_UNSEEN = [0, 12, 16, 18], [16, 18]


class Ragged(torch.utils.data.Dataset):
    """native synthetic samples of two sizes, alternating"""

    def __init__(self, n=4):
        self.parts = [SyntheticSegmentation(n_images=n, size=s, n_class=K, embed_dim=E, seed=5 + i, native=True)
                      for i, s in enumerate([(48, 56), (72, 40)])]
        self.class_names = self.parts[0].class_names
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return self.parts[i % 2][i]


def new_model():
    m = models.FCN32s(E)
    m.load_synthetic(1337, device=torch.device("cuda"))
    return m


def loaders():
    train_loader = torch.utils.data.DataLoader(Ragged(), batch_size=2, shuffle=False, collate_fn=datasets.augment_collate)
    val = SyntheticSegmentation(split="val", n_images=1, size=(48, 56), n_class=K, embed_dim=E, seed=5)
    return train_loader, torch.utils.data.DataLoader(val, batch_size=1, shuffle=False)


def spy_augment_kernels(monkeypatch):
    """(entry, szn_last_kernel() right after it) of every augmentation call"""
    seen = []
    real = L.call

    def call(name, *a):
        out = real(name, *a)
        if name.startswith("szn_augment"):
            seen.append((name, L.last_kernel()))
        return out
    monkeypatch.setattr(L, "call", call)
    return seen


def affine_augment():
    return datasets.Augment((64, 64), (0.5, 2.0), rotate=10.0, jitter=JITTER)


def test_trainer_fcn_trains_on_rotated_jittered_crops(tmp_path, monkeypatch):
    m = new_model()
    train_loader, val_loader = loaders()
    ws = [getattr(m, n).weight for n in models._OPT_LAYERS]
    bs = [getattr(m, n).bias for n in models._OPT_LAYERS]
    opt = optim.FusedAdam([{"params": ws}, {"params": bs, "lr": 2e-5}], lr=1e-5)
    t = trainer_fcn.Trainer(cuda=True, model=m, optimizer=opt, train_loader=train_loader, val_loader=val_loader, log_dir=str(tmp_path),
                            dataset="context", max_epoch=1, tb_writer=None, pixel_embeddings=E, loss_func="cos", unseen=UNSEEN,
                            val_unseen=VAL_UNSEEN, augment=affine_augment())
    assert isinstance(t._fast_step(), engine.TrainStep)
    seen = spy_augment_kernels(monkeypatch)
    t.train_epoch()
    assert t.iteration == 2 and seen == [("szn_augment_affine_u8", "augment_affine_u8_kernel_v4")] * 2
    rows = open(os.path.join(str(tmp_path), "train_log.csv")).read().strip().split("\n")
    assert len(rows) == 1 + 2 and all(np.isfinite(float(r.split(",")[2])) for r in rows[1:])


def test_trainer_seenmask_trains_on_rotated_jittered_crops(tmp_path, monkeypatch):
    model = new_model()
    train_loader, val_loader = loaders()
    head = list(model.seenmask_score.parameters()) + list(model.seenmask_upscore.parameters())
    st = trainer_seenmask.Trainer(cuda=True, model=model, optimizer=optim.FusedAdam(head, lr=1e-3), train_loader=train_loader,
                                  val_loader=val_loader, log_dir=str(tmp_path), dataset="context", max_epoch=1, tb_writer=None,
                                  checkpoint={}, unseen=[0, 12], augment=affine_augment())
    assert isinstance(st._fast_step(), engine.SeenmaskStep)
    seen = spy_augment_kernels(monkeypatch)
    st.train_epoch()
    assert seen == [("szn_augment_affine_u8", "augment_affine_u8_kernel_v4")] * 2
    rows = open(os.path.join(str(tmp_path), "seenmask_train_log.csv")).read().strip().split("\n")
    assert len(rows) == 1 + 2 and all(np.isfinite(float(r.split(",")[2])) for r in rows[1:])


def test_train_cli_rotate_and_color_jitter(fast_tmp, monkeypatch):
    d = fast_tmp
    with pytest.raises((Exception, SystemExit)):
        train.main(['-c', '18', '-ve', '1', '-dir', d, '-n', 'bad', '--synthetic', '4', '96', '128', '--batch-size', '2', '--rotate', '10',
                    '--workers', '0'])
    assert not glob.glob(os.path.join(d, 'logs', 'bad_CFG_18_*'))
    seen = spy_augment_kernels(monkeypatch)
    train.main(['-c', '18', '-ve', '1', '-dir', d, '-n', 'affine', '--synthetic', '4', '96', '128', '--batch-size', '2', '--precision', 'bf16',
                '--crop-size', '64', '64', '--rotate', '10', '--color-jitter', '0.125', '0.5', '0.5', '18', '--workers', '0'])
    log = glob.glob(os.path.join(d, 'logs', 'affine_CFG_18_*'))
    assert len(log) == 1
    rows = open(os.path.join(log[0], 'train_log.csv')).read().strip().split('\n')
    assert len(rows) == 1 + 2 and all(np.isfinite(float(r.split(',')[2])) for r in rows[1:])        # 4 images, batches of 2, 1 epoch
    assert os.path.exists(os.path.join(log[0], 'val_log.csv')) and os.path.exists(os.path.join(log[0], 'seenmask_train_log.csv'))
    assert seen and {s[0] for s in seen} == {"szn_augment_affine_u8"}                                 # both phases, never the plain kernel
