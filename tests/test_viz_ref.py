"""CPU: the numpy restatement of the visualisation contract (tests/helpers_viz.py) against independent anchors -- literal PASCAL colours,
PIL's grey conversion, the byte round trip through the dataset transform, helpers_state's counter-based generator -- plus the host-side
surface of the feature (mosaic shape, train.py --viz, the reference's names in vis_utils).  The MI355X side is tests/test_gpu_viz.py."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers_state as HS  # noqa: E402
import helpers_viz as HV  # noqa: E402


def test_colour_map_literals():
    cmap = HV.colormap(256)
    want = {0: (0, 0, 0), 1: (128, 0, 0), 2: (0, 128, 0), 15: (192, 128, 128), 20: (0, 64, 128), 255: (224, 224, 192)}
    for k, rgb in want.items():
        assert tuple(cmap[k]) == rgb, (k, tuple(cmap[k]))
    assert len({tuple(c) for c in cmap}) == 256                   # a bit shuffle: no two classes share a colour
    lbl = np.array([[-1, 0, 1], [20, 21, 300]])
    assert np.array_equal(HV.colour(lbl, 21), np.array([[(0, 0, 0), (0, 0, 0), (128, 0, 0)], [(0, 64, 128), (0, 0, 0), (0, 0, 0)]]))


def test_package_colour_map_equals_restatement():
    from zeroshotsemanticsegmentation_amd import vis_utils
    assert np.array_equal(vis_utils.label_colormap(256), HV.colormap(256))
    assert vis_utils.label_colormap(21).shape == (21, 3) and vis_utils.label_colormap(21).dtype == np.uint8


def test_grey_equals_pil():
    from PIL import Image
    img = np.random.RandomState(3).randint(0, 256, (64, 64, 3)).astype(np.uint8)
    img[0, 0], img[0, 1], img[0, 2] = (255, 255, 255), (0, 0, 0), (255, 0, 0)
    assert np.array_equal(HV.grey(img), np.asarray(Image.fromarray(img).convert('L')))
    assert HV.grey(img)[0, 0] == 255 and HV.grey(img)[0, 1] == 0 and HV.grey(img)[0, 2] == 76


def test_overlay_is_half_colour_half_grey():
    col = np.arange(256, dtype=np.uint8).reshape(-1, 1, 1).repeat(256, 1).repeat(3, 2)      # every (colour, grey) pair
    g = np.arange(256, dtype=np.uint8).reshape(1, -1).repeat(256, 0)
    assert np.array_equal(HV.overlay(col, g), (0.5 * col + 0.5 * g[..., None]).astype(np.uint8))


def test_rounding_recovers_every_byte_and_truncation_does_not():
    """the stated deviation from dataset.untransform: u - mean -> f32 -> + mean is below u for most (value, channel) pairs"""
    u = np.arange(256, dtype=np.uint8).reshape(1, 256, 1, 1).repeat(3, 3)                   # (1,256,1,3): every value in every channel
    x = HV.transform(u)
    assert np.array_equal(HV.recover(x, rounding=True), u)
    bad = HV.recover(x, rounding=False) != u
    assert bad.sum() == 568 and np.all(HV.recover(x, rounding=False)[bad] == u[bad] - 1)
    # out-of-range inputs clamp
    far = np.array([-1000.0, 1000.0, 0.0], np.float32).reshape(1, 3, 1, 1)
    assert np.array_equal(HV.recover(far)[0, 0, 0], [123, 255, 0])                           # RGB <- BGR (0+122.68 | 1000 | -1000)


def test_noise_equals_state_generator():
    """byte = floor(u * 255) with u the 24-bit uniform helpers_state.dropout_ref thresholds: byte >= m  <=>  u >= ceil(m * 2^24 / 255) / 2^24
    (a float32-exact p), so the byte is the number of thresholds m = 1..254 the Dropout2d restatement keeps the counter at"""
    B, H, W, seed = 2, 3, 5, 1337
    n = B * H * W * 3
    got = HV.noise(B, H, W, seed).reshape(-1).astype(np.int64)
    want = np.zeros(n, np.int64)
    for m in range(1, 255):
        p = -(-(m << 24) // 255) / float(1 << 24)
        assert float(np.float32(p)) == p and p < 1
        want += HS.dropout_ref(n, p, seed, 0) != 0
    assert np.array_equal(got, want) and got.max() <= 254
    assert not np.array_equal(got, HV.noise(B, H, W, seed + 1).reshape(-1))
    assert np.array_equal(HV.noise_counters(B, H, W).reshape(-1), np.arange(n))


def test_layouts_on_a_hand_made_image():
    img = np.full((1, 1, 2, 3), 200, np.uint8)
    lt, lp = np.array([[[1, -1]]]), np.array([[[2, 1]]])
    v = HV.segmentation(img, lt, lp, 21, unseen=[2], seed=7)
    assert v.shape == (1, 2, 8, 3)
    nz = HV.noise(1, 1, 2, 7)[0, 0, 1]
    assert np.array_equal(v[0, 0, :, 0], [200, 200, 128, nz[0], (128 + 200) >> 1, nz[0], 255, nz[0]])
    assert np.array_equal(v[0, 1, :, 1], [200, 200, 128, nz[1], (128 + 200) >> 1, nz[1], 0, nz[1]])      # class 2 is unseen: mask 0
    assert HV.segmentation(img, lt, lp, 21).shape == (1, 2, 6, 3)
    only_pred = HV.segmentation(img, None, lp, 21, unseen=[2])
    assert only_pred.shape == (1, 1, 8, 3) and np.array_equal(only_pred[0, 0, :, 0], [200, 200, 0, 128, 100, 164, 0, 255])
    s = HV.seenmask(img, np.array([[[1, -2]]]), np.array([[[0, 1]]]), seed=7)
    assert s.shape == (1, 1, 6, 3) and np.array_equal(s[0, 0, :, 2], [200, 200, 255, nz[2], 0, nz[2]])


def test_tile_shape_and_mosaic():
    from zeroshotsemanticsegmentation_amd import vis_utils
    want = {1: (1, 1), 2: (1, 2), 3: (1, 3), 5: (2, 3), 25: (5, 5)}
    for n, shape in want.items():
        assert HV.tile_shape(n) == shape and vis_utils.mosaic_shape(n) == shape
    a, b = np.full((2, 4, 3), 9, np.uint8), np.full((4, 2, 3), 7, np.uint8)
    m = HV.mosaic([a, b])
    assert m.shape == (4, 8, 3) and m.sum() == 9 * a.size + 7 * b.size
    assert np.all(m[1:3, 0:4] == 9) and np.all(m[:, 5:7] == 7)


def test_train_cli_knows_viz():
    from zeroshotsemanticsegmentation_amd import train
    p = train.build_parser()
    assert p.parse_args([]).viz == 0
    assert p.parse_args(['--viz', '25']).viz == 25


def test_vis_utils_exposes_reference_names():
    import pytest
    from zeroshotsemanticsegmentation_amd import vis_utils
    for name in ("visualize_segmentation", "visualize_seenmask", "make_seen_mask", "visualize_segmentation_device",
                 "visualize_seenmask_device", "get_tile_image", "label_colormap"):
        assert callable(getattr(vis_utils, name)), name
    with pytest.raises(RuntimeError, match="Unexpected keys"):
        vis_utils.visualize_segmentation(img=None, colour="red")
    with pytest.raises(RuntimeError, match="Unexpected keys"):
        vis_utils.visualize_seenmask(img=None, colour="red")
