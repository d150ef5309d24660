"""CPU: the numpy restatement of the augmentation contract (tests/helpers_augment.py) against independent anchors -- the dataset transform
of datasets.py, np.flip, exact 2x2 block means, constancy, torch's own bilinear interpolation within a derived bound -- plus the host side
of the feature: datasets.Augment's records, augment_collate, the native synthetic samples and train.py's flags.  The MI355X side is
tests/test_gpu_augment.py."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers_augment as HA  # noqa: E402

MEAN = np.array(HA.MEAN_BGR)


def sample(h, w, seed, B=1):
    rng = np.random.RandomState(seed)
    img = rng.randint(0, 256, (B, h, w, 3)).astype(np.uint8)
    lbl = rng.randint(-1, 21, (B, h, w)).astype(np.int64)
    return img, lbl


def transform(img):
    """datasets._SegmentationDataset.transform on a batch"""
    return (img[..., ::-1].astype(np.float64) - MEAN).astype(np.float32).transpose(0, 3, 1, 2)


def test_identity_is_the_dataset_transform():
    img, lbl = sample(7, 9, 0, B=2)
    rec = [HA.record(7, 9, 1.0)] * 2
    assert rec[0] == [7, 9, 7, 9, 65536, 65536, 0, 0, 0]
    data, target = HA.augment(img, lbl, rec, (7, 9))
    assert data.dtype == np.float32 and np.array_equal(data, transform(img))
    assert target.dtype == np.int64 and np.array_equal(target, lbl)


def test_flip_is_np_flip():
    img, lbl = sample(6, 11, 1)
    d0, t0 = HA.augment(img, lbl, [HA.record(6, 11, 1.0)], (6, 11))
    d1, t1 = HA.augment(img, lbl, [HA.record(6, 11, 1.0, flip=True)], (6, 11))
    assert np.array_equal(d1, np.flip(d0, axis=3)) and np.array_equal(t1, np.flip(t0, axis=2))


def test_halving_is_the_exact_2x2_mean():
    img, lbl = sample(8, 12, 2)
    rec = HA.record(8, 12, 0.5)
    assert rec[2:6] == [4, 6, 131072, 131072]
    v, lab, pad = HA.fixed_point(img[0], lbl[0], rec, (4, 6))
    blocks = img[0].astype(np.int64).reshape(4, 2, 6, 2, 3).sum(axis=(1, 3))
    assert np.array_equal(v, blocks << 20) and not pad.any()                  # weights 1024 / 2048 on both axes: sum / 4, exactly
    data, _ = HA.augment(img, lbl, [rec], (4, 6))
    want = (blocks[:, :, ::-1] / 4.0 - MEAN).astype(np.float32).transpose(2, 0, 1)
    assert np.array_equal(data[0], want)
    assert np.array_equal(lab, lbl[0][1::2, 1::2])                            # nearest of a centre between four pixels: the lower right


@pytest.mark.parametrize("s", [0.5, 0.77, 1.0, 4 / 3, 2.0])
def test_constant_image_stays_constant(s):
    img = np.full((1, 5, 7, 3), 0, dtype=np.uint8)
    img[..., 0], img[..., 1], img[..., 2] = 255, 17, 1
    rec = HA.record(5, 7, s)
    v, _, pad = HA.fixed_point(img[0], np.zeros((5, 7), np.int64), rec, (rec[2], rec[3]))
    assert not pad.any() and np.array_equal(v, np.broadcast_to(np.array([255, 17, 1], dtype=np.int64) << 22, v.shape))


def test_against_torch_bilinear():
    """align_corners=False, no antialiasing, float64 on the CPU; the bound is derived in helpers_augment's docstring and not tuned"""
    worst = 0.0
    for seed, (h, w) in enumerate([(13, 17), (16, 9), (31, 24)]):
        img, lbl = sample(h, w, 10 + seed)
        x = torch.from_numpy(img[0].astype(np.float64)).permute(2, 0, 1)[None]
        for s in (0.5, 0.6, 0.77, 1.0, 1.3, 1.5, 1.9, 2.0):
            rec = HA.record(h, w, s)
            Hs, Ws = rec[2], rec[3]
            v, _, pad = HA.fixed_point(img[0], lbl[0], rec, (Hs, Ws))
            ref = torch.nn.functional.interpolate(x, size=(Hs, Ws), mode='bilinear', align_corners=False, antialias=False)
            err = np.abs(v / 4194304.0 - ref[0].permute(1, 2, 0).numpy()).max()
            bound = HA.interp_bound(Hs, Ws)
            print("h %d w %d s %.2f -> %d x %d: max |diff| %.5f, bound %.5f" % (h, w, s, Hs, Ws, err, bound))
            assert not pad.any() and err < bound, (h, w, s, err, bound)
            worst = max(worst, err / bound)
    print("largest measured / bound: %.3f" % worst)


def test_padding_and_window():
    img, lbl = sample(5, 7, 3)
    rec = HA.record(5, 7, 1.0, oy=-2, ox=3)
    data, target = HA.augment(img, lbl, [rec], (9, 8))
    want_l = np.full((9, 8), HA.PAD_LABEL, dtype=np.int64)
    want_l[2:7, 0:4] = lbl[0][:, 3:7]
    assert np.array_equal(target[0], want_l)
    assert np.all(data[0][:, want_l == HA.PAD_LABEL] == 0.0)
    assert np.array_equal(data[0][:, 2:7, 0:4], transform(img)[0][:, :, 3:7])


# ---- the package's host side -------------------------------------------------------------------------------------------------------
def test_augment_params_reproducible_and_keyed():
    from zeroshotsemanticsegmentation_amd import datasets
    from zeroshotsemanticsegmentation_amd._lib import AUG_NPARAM
    assert AUG_NPARAM == HA.NPARAM and datasets.PAD_LABEL == HA.PAD_LABEL
    sizes = np.array([(375, 500), (333, 500), (500, 281), (40, 30)])
    aug = datasets.Augment((128, 160), (0.5, 2.0))
    a = aug.params(sizes, epoch=3, iteration=17, rank=1)
    assert a.dtype == np.int32 and a.shape == (4, HA.NPARAM)
    assert np.array_equal(a, datasets.Augment((128, 160), (0.5, 2.0)).params(torch.from_numpy(sizes), 3, 17, 1))
    for other in (aug.params(sizes, 3, 17, 0), aug.params(sizes, 3, 18, 1), aug.params(sizes, 4, 17, 1),
                  datasets.Augment((128, 160), (0.5, 2.0), seed=7).params(sizes, 3, 17, 1)):
        assert not np.array_equal(a, other)
    # image i's draw does not depend on its neighbours
    assert np.array_equal(aug.params(sizes[:2], 3, 17, 1), a[:2])


def test_augment_params_ranges():
    from zeroshotsemanticsegmentation_amd import datasets
    Hc, Wc = 96, 128
    aug = datasets.Augment((Hc, Wc), (0.5, 2.0))
    sizes = np.array([(100, 140), (60, 200), (375, 500), (30, 20)])
    flips, seen_scales, big = [], [], 0
    for it in range(200):
        for (h, w), r in zip(sizes, aug.params(sizes, 0, it)):
            h_, w_, Hs, Ws, sy, sx, oy, ox, flip = [int(v) for v in r]
            assert (h_, w_) == (h, w) and flip in (0, 1)
            assert np.floor(0.5 * h + 0.5) <= Hs <= np.floor(2.0 * h + 0.5) and np.floor(0.5 * w + 0.5) <= Ws <= np.floor(2.0 * w + 0.5)
            assert abs(Hs / h - Ws / w) <= 0.5 / h + 0.5 / w + 1e-12                                  # one isotropic scale
            assert sy == ((h << 16) + Hs // 2) // Hs and sx == ((w << 16) + Ws // 2) // Ws
            assert 0 <= oy <= max(Hs - Hc, 0) and 0 <= ox <= max(Ws - Wc, 0)
            assert (oy == 0 or Hs > Hc) and (ox == 0 or Ws > Wc)
            big += Hs > Hc and oy > 0
            flips.append(flip)
            seen_scales.append(Hs / h)
    assert 0.3 < np.mean(flips) < 0.7 and big > 50
    assert min(seen_scales) < 0.6 and max(seen_scales) > 1.9 and 1.1 < np.mean(seen_scales) < 1.4       # U[0.5, 2]: mean 1.25
    # the largest origin is reachable: a 1-pixel range takes both values
    one = datasets.Augment((10, 10), (1.0, 1.0), flip=False)
    got = {tuple(one.params([(11, 11)], 0, it)[0, 6:8]) for it in range(64)}
    assert got == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_augment_params_identity_record():
    from zeroshotsemanticsegmentation_amd import datasets
    aug = datasets.Augment((16, 16), (1.0, 1.0), flip=False)
    sizes = [(7, 9), (16, 16), (1, 1)]
    for it in range(5):
        assert np.array_equal(aug.params(sizes, 0, it), np.array([HA.record(h, w, 1.0) for h, w in sizes], dtype=np.int32))
    assert np.array_equal(aug.params(sizes, 0, 0)[0], [7, 9, 7, 9, 65536, 65536, 0, 0, 0])
    with pytest.raises(ValueError):
        datasets.Augment((0, 16))
    with pytest.raises(ValueError):
        datasets.Augment((16, 16), (2.0, 0.5))


def test_augment_collate_and_native_synthetic_samples():
    from zeroshotsemanticsegmentation_amd import datasets, synth
    from zeroshotsemanticsegmentation_amd.synthetic_dataset import SyntheticSegmentation
    a = SyntheticSegmentation(n_images=2, size=(6, 9), n_class=33, embed_dim=20, seed=5, native=True)
    b = SyntheticSegmentation(n_images=2, size=(8, 5), n_class=33, embed_dim=20, seed=6, native=True)
    img, lbl = a[1]
    assert img.dtype == torch.uint8 and tuple(img.shape) == (6, 9, 3) and lbl.dtype == torch.int64 and tuple(lbl.shape) == (6, 9)
    # the bytes the float sample is made from: the default sample is their dataset transform
    f_img, (f_lbl, _) = SyntheticSegmentation(n_images=2, size=(6, 9), n_class=33, embed_dim=20, seed=5)[1]
    assert np.array_equal(transform(img.numpy()[None])[0], f_img.numpy()) and torch.equal(lbl, f_lbl)
    assert np.array_equal(f_img.numpy(), synth.make_images(1, 6, 9, seed=5 + 1)[0])
    batch = [a[0], b[0]]
    ci, cl, sizes = datasets.augment_collate(batch)
    pi, pl = datasets.pad_collate(batch)
    assert torch.equal(ci, pi) and torch.equal(cl, pl) and tuple(ci.shape) == (2, 8, 9, 3)
    assert sizes.dtype == torch.int32 and sizes.tolist() == [[6, 9], [8, 5]]


def test_parser_knows_the_flags():
    from zeroshotsemanticsegmentation_amd import train
    p = train.build_parser()
    d = p.parse_args([])
    assert d.crop_size is None and list(d.scale_range) == [0.5, 2.0] and d.no_flip is False
    a = p.parse_args(['--crop-size', '64', '96', '--scale-range', '0.75', '1.5', '--no-flip'])
    assert list(a.crop_size) == [64, 96] and list(a.scale_range) == [0.75, 1.5] and a.no_flip is True
