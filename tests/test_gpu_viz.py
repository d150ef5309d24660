"""GPU: the visualisation kernel (csrc/szn_viz.hip), its Python surface (vis_utils) and the trainers' per-epoch picture against the numpy
restatement of the contract in tests/helpers_viz.py.  The contract is integer-exact: every comparison is np.array_equal.

Shapes: 37 x 45 (byte path: 3W is no multiple of 4, the last 4-pixel run of a row holds one pixel, 2 blocks), 3 x 64 (dword-store
path) and 1 x 1; class sets on both sides of the 64- and 128-bit word boundaries of szn_class_set."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers_viz as HV  # noqa: E402
from zeroshotsemanticsegmentation_amd import _lib as L  # noqa: E402
from zeroshotsemanticsegmentation_amd import models, optim, trainer_fcn, trainer_seenmask, vis_utils  # noqa: E402
from zeroshotsemanticsegmentation_amd.synthetic_dataset import SyntheticSegmentation  # noqa: E402

B = 2
SHAPES = {(37, 45): "viz_panels_kernel", (3, 64): "viz_panels_kernel_v4", (1, 1): "viz_panels_kernel"}
SETS = {"k21": (21, [0, 6, 20]), "k150": (150, [0, 63, 64, 65, 127, 128, 129, 149]), "nomask": (21, None)}
SEED = 4242


@functools.lru_cache(maxsize=None)
def inputs(H, W, K):
    """uint8 image, its network-input form, truth with -1 / -2 / >= K pixels, a prediction that uses every class (as far as B*H*W goes)"""
    rng = np.random.RandomState(1000 * H + W + K)
    img = rng.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    img.reshape(-1, 3)[:2] = [(255, 255, 255), (0, 0, 0)]
    lt = rng.randint(0, K, (B, H, W)).astype(np.int64)
    n = lt.size
    flat = lt.reshape(-1)
    flat[0] = -1
    if n > 8:
        flat[rng.choice(n, n // 7, replace=False)] = -1
        flat[rng.choice(n, n // 9, replace=False)] = -2
        flat[rng.choice(n, 5, replace=False)] = [K, K + 1, 255, 256, 2 ** 40]
        flat[-1] = -1                                           # the last pixel of the batch: the last thread's partial run
    lp = rng.permutation(np.arange(n) % K).reshape(B, H, W).astype(np.int64)
    if n > 8:
        lp.reshape(-1)[rng.choice(n, 3, replace=False)] = [-1, K, 2 ** 33]     # a prediction outside [0, K) is black, not noise
    for a in (img, lt, lp):
        a.setflags(write=False)
    return img, HV.transform(img), lt, lp


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


@pytest.mark.parametrize("cfg", sorted(SETS))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_segmentation_equals_contract(shape, cfg):
    H, W = shape
    K, unseen = SETS[cfg]
    img, x, lt, lp = inputs(H, W, K)
    want = HV.segmentation(img, lt, lp, K, unseen, SEED)
    n_col = 4 if unseen else 3
    assert want.shape == (B, 2 * H, n_col * W, 3)
    if H * W > 8:
        assert set(np.unique(lp)) >= set(range(K)) and (lt < 0).any() and (lt >= K).any()
    got = {}
    for kind, data in (("u8", img), ("f32", x)):
        out = vis_utils.visualize_segmentation_device(dev(data), dev(lt), dev(lp), K, unseen=unseen, seed=SEED)
        assert L.last_kernel() == SHAPES[shape]
        assert out.dtype == torch.uint8 and tuple(out.shape) == want.shape
        got[kind] = out.cpu().numpy()
        assert np.array_equal(got[kind], want), kind
    assert np.array_equal(got["u8"], got["f32"])
    # another seed moves the noise and nothing else
    other = vis_utils.visualize_segmentation_device(dev(img), dev(lt), dev(lp), K, unseen=unseen, seed=SEED + 1).cpu().numpy()
    assert np.array_equal(other, HV.segmentation(img, lt, lp, K, unseen, SEED + 1))
    unl = np.tile((lt < 0) | (lt >= K), (1, 2, n_col))
    unl[:, :, :W] = False
    assert np.array_equal(other[~unl], want[~unl]) and not np.array_equal(other[unl], want[unl])


@pytest.mark.parametrize("shape,x_off,kernel", [((37, 45), 4, "viz_panels_kernel"), ((3, 64), 4, "viz_panels_kernel_v4"),
                                                ((3, 64), 1, "viz_panels_kernel")])
def test_render_into_a_canvas_writes_only_the_panels(shape, x_off, kernel):
    """out_row_bytes / out_image_bytes larger than needed: the picture lands at its offset in a 0xA5 canvas and every other byte stays.
    3 x 64 at a 4-pixel offset keeps every store dword-aligned; at a 1-pixel offset `out` is not, and the byte kernel takes over."""
    H, W = shape
    K, unseen = SETS["k21"]
    img, x, lt, lp = inputs(H, W, K)
    want = HV.segmentation(img, lt, lp, K, unseen, SEED)
    canvas = torch.full((B, 2 * H + 5, 4 * W + 8, 3), 0xA5, dtype=torch.uint8, device="cuda")
    view = canvas[:, 2:2 + 2 * H, x_off:x_off + 4 * W]
    ret = vis_utils.visualize_segmentation_device(dev(x), dev(lt), dev(lp), K, unseen=unseen, seed=SEED, out=view)
    assert L.last_kernel() == kernel and ret.data_ptr() == view.data_ptr()
    c = canvas.cpu().numpy()
    assert np.array_equal(c[:, 2:2 + 2 * H, x_off:x_off + 4 * W], want)
    c[:, 2:2 + 2 * H, x_off:x_off + 4 * W] = 0xA5
    assert np.all(c == 0xA5)


def test_without_truth_only_the_prediction_row_and_no_noise():
    H, W = 37, 45
    K, unseen = SETS["k150"]
    img, x, lt, lp = inputs(H, W, K)
    out = vis_utils.visualize_segmentation_device(dev(img), None, dev(lp), K, unseen=unseen, seed=SEED).cpu().numpy()
    assert out.shape == (B, H, 4 * W, 3)
    assert np.array_equal(out, HV.segmentation(img, None, lp, K, unseen, SEED))
    assert np.array_equal(out, HV.segmentation(img, None, lp, K, unseen, SEED + 1))                # nothing depends on the seed
    # and it is the prediction row of the two-row picture wherever the truth is labelled
    both = HV.segmentation(img, lt, lp, K, unseen, SEED)[:, H:]
    lab = np.tile((lt >= 0) & (lt < K), (1, 1, 4))
    assert np.array_equal(out[lab], both[lab])


def test_seenmask_layout_equals_contract():
    H, W = 37, 45
    img, x, _, _ = inputs(H, W, 21)
    rng = np.random.RandomState(9)
    lt = rng.randint(0, 2, (B, H, W)).astype(np.int64)
    lt.reshape(-1)[rng.choice(lt.size, 200, replace=False)] = -2
    lt.reshape(-1)[rng.choice(lt.size, 50, replace=False)] = -1
    lp = rng.randint(0, 2, (B, H, W)).astype(np.int64)
    want = HV.seenmask(img, lt, lp, SEED)
    for data in (img, x):
        out = vis_utils.visualize_seenmask_device(dev(data), dev(lt), dev(lp), seed=SEED)
        assert L.last_kernel() == "viz_panels_kernel" and tuple(out.shape) == (B, H, 3 * W, 3)
        assert np.array_equal(out.cpu().numpy(), want)
    x4 = np.ascontiguousarray(x[:, :, :, :44])
    out = vis_utils.visualize_seenmask_device(dev(x4), dev(lt[:, :, :44]), dev(lp[:, :, :44]), seed=SEED)
    assert L.last_kernel() == "viz_panels_kernel_v4"
    assert np.array_equal(out.cpu().numpy(), HV.seenmask(x4, lt[:, :, :44], lp[:, :, :44], SEED))


def test_argument_errors():
    H, W = 3, 64
    img, x, lt, lp = inputs(H, W, 21)
    d, t, p = dev(img), dev(lt), dev(lp)
    for K, unseen in ((0, None), (257, None), (21, [21]), (21, [3, 200])):
        with pytest.raises(L.SznError):
            vis_utils.visualize_segmentation_device(d, t, p, K, unseen=unseen)
    out = torch.empty(B, 2 * H, 4 * W, 3, dtype=torch.uint8, device="cuda")
    mean = (C.c_double * 3)(*HV.MEAN_BGR)
    row, image = 3 * 4 * W, 2 * H * 3 * 4 * W

    def call(row_bytes, image_bytes, img_ptr=L.ptr(d), kind=0, mean_arg=mean):
        L.call("szn_viz_segmentation", B, H, W, img_ptr, kind, mean_arg, L.ptr(t), L.ptr(p), 21, L.class_set([0, 6]), SEED, L.ptr(out), row_bytes,
               image_bytes, L.stream_ptr())
    call(row, image)                                            # the dense picture is accepted ...
    for bad in ((row - 1, image), (row, image - 1), (row, image, None), (row, image, L.ptr(d), 2), (row, image, L.ptr(d), 1, None)):
        with pytest.raises(L.SznError):                         # ... a short row, a short image, no image, an unknown kind, kind 1 without mean
            call(*bad)
    with pytest.raises(L.SznError):
        L.call("szn_viz_seenmask", B, H, W, L.ptr(d), 0, mean, L.ptr(t), L.ptr(p), SEED, L.ptr(out), 3 * 3 * W - 1, image, L.stream_ptr())
    with pytest.raises(L.SznError):
        L.call("szn_viz_seenmask", B, H, W, L.ptr(d), 0, mean, None, L.ptr(p), SEED, L.ptr(out), row, image, L.stream_ptr())
    with pytest.raises(L.SznError):
        vis_utils.visualize_segmentation_device(d.cpu(), t, p, 21)                      # no CPU drawing path


def test_reference_named_wrappers():
    H, W = 37, 45
    K, unseen = SETS["k21"]
    img, x, lt, lp = inputs(H, W, K)
    i0, t0, p0 = img[0].copy(), lt[0].copy(), lp[0].copy()
    t0[t0 > 2 ** 31] = -1
    p0[p0 > 2 ** 31] = 0
    t1, p1 = t0.astype(np.int32), p0.astype(np.int32)           # the datasets hand out int32 labels: any integer type is taken
    keep = t1.copy(), p1.copy()
    got = vis_utils.visualize_segmentation(img=i0, lbl_true=t1, lbl_pred=p1, n_class=K, unseen=unseen, label_names=["x"] * K)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8
    assert np.array_equal(got, HV.segmentation(i0[None], t0[None], p0[None], K, unseen, 1337)[0])
    assert np.array_equal(t1, keep[0]) and np.array_equal(p1, keep[1])                  # the reference zeroes lbl_true in place
    got3 = vis_utils.visualize_segmentation(img=i0, lbl_true=t1, lbl_pred=p1, n_class=K)
    assert np.array_equal(got3, HV.segmentation(i0[None], t0[None], p0[None], K, None, 1337)[0])
    bt, bp = (t0 % 2).astype(np.int64), (p0 % 2).astype(np.int64)
    bt[t0 < 0] = -1
    keep = bt.copy(), bp.copy()
    got = vis_utils.visualize_seenmask(img=i0, lbl_true=bt, lbl_pred=bp, unseen=[0], n_class=2)
    assert np.array_equal(got, HV.seenmask(i0[None], bt[None], bp[None], 1337)[0])
    assert np.array_equal(bt, keep[0]) and np.array_equal(bp, keep[1])
    assert np.array_equal(vis_utils.make_seen_mask(t0, unseen, K), HV.mask(t0, K, unseen))
    assert np.array_equal(vis_utils.make_seen_mask(t0, [], K), HV.mask(t0, K, []))


def test_mosaic_of_three_sizes():
    rng = np.random.RandomState(5)
    tiles = [rng.randint(1, 256, s + (3,)).astype(np.uint8) for s in ((6, 10), (9, 4), (3, 3))]
    got = vis_utils.get_tile_image([dev(t) for t in tiles])
    assert got.is_cuda and tuple(got.shape) == (9, 30, 3)
    assert np.array_equal(got.cpu().numpy(), HV.mosaic(tiles))
    five = vis_utils.get_tile_image([dev(tiles[0])] * 5)
    assert tuple(five.shape) == (12, 30, 3) and np.array_equal(five.cpu().numpy(), HV.mosaic([tiles[0]] * 5))


# ---- end to end: the trainers' per-epoch picture ----------------------------------------------------------------------------------
E, K, H, W = 20, 21, 64, 64
UNSEEN, VAL_UNSEEN = [3, 6, 20], [6, 20]


@pytest.fixture(scope="module")
def net():
    m = models.FCN32s(E)
    m.load_synthetic(1337, device=torch.device("cuda"))
    ds = SyntheticSegmentation(split="val", n_images=4, size=(H, W), n_class=K, embed_dim=E, seed=5)
    return m, torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False)


def fcn_trainer(net, tmp, visualize):
    m, loader = net
    ws = [getattr(m, n).weight for n in models._OPT_LAYERS]
    bs = [getattr(m, n).bias for n in models._OPT_LAYERS]
    opt = optim.FusedAdam([{"params": ws}, {"params": bs, "lr": 2e-5}], lr=1e-5)
    return trainer_fcn.Trainer(cuda=True, model=m, optimizer=opt, train_loader=loader, val_loader=loader, log_dir=str(tmp),
                               dataset="pascal", max_epoch=1, tb_writer=None, pixel_embeddings=E, loss_func="cos", unseen=UNSEEN,
                               val_unseen=VAL_UNSEEN, precision=torch.float32, visualize=visualize)


class _Writer(object):
    def __init__(self):
        self.images = []

    def add_scalar(self, *a, **k): pass
    def add_text(self, *a, **k): pass

    def add_image(self, tag, img, step, dataformats='CHW'):
        self.images.append((tag, img, step, dataformats))


def test_fcn_trainer_writes_the_epoch_picture(net, tmp_path):
    from PIL import Image
    m, loader = net
    t = fcn_trainer(net, tmp_path, 2)
    t.tb_writer = tb = _Writer()
    t.validate()
    path = os.path.join(str(tmp_path), "fcn_viz", "epoch0.jpg")
    assert os.path.exists(path) and Image.open(path).size == (2 * 4 * W, 2 * H)         # 2 tiles of (2H, 4W) side by side; PIL: (w, h)
    assert t.last_viz.shape == (2 * H, 2 * 4 * W, 3) and t.last_viz.dtype == np.uint8
    assert len(tb.images) == 1 and tb.images[0][0] == 'fcn/segmentations' and tb.images[0][3] == 'HWC' and tb.images[0][1] is t.last_viz
    m.eval()
    tiles = []
    for i, (data, target) in enumerate(loader):
        if i == 2:
            break
        lbl = target[0]
        with torch.no_grad():
            _, pred = m.embed_predict(data.cuda(), t.embeddings, lbl.cuda(), loss="cos")
        tiles.append(HV.segmentation(data.numpy(), lbl.numpy(), pred.cpu().numpy(), K, VAL_UNSEEN, 1337, np.asarray(loader.dataset.mean_bgr))[0])
        if i == 0:
            assert (lbl.numpy() < 0).any()                                               # the synthetic truth has unlabelled pixels: noise is on
            first = t.last_viz[:, :4 * W]
            assert np.array_equal(first[:H, :W], HV.recover(data.numpy())[0])           # the rounded-untransformed input
            assert np.array_equal(first[:H], tiles[0][:H])                               # truth panels
            assert np.array_equal(first[H:], tiles[0][H:])                               # prediction panels
    assert np.array_equal(t.last_viz, HV.mosaic(tiles))


def test_fcn_trainer_without_visualize_writes_nothing(net, tmp_path):
    t = fcn_trainer(net, tmp_path, 0)
    t.validate()
    assert t.last_viz is None and not os.path.exists(os.path.join(str(tmp_path), "fcn_viz"))
    assert os.path.exists(os.path.join(str(tmp_path), "val_log.csv"))


def test_seenmask_trainer_writes_the_epoch_picture(net, tmp_path):
    from PIL import Image
    m, loader = net
    head = list(m.seenmask_score.parameters()) + list(m.seenmask_upscore.parameters())
    st = trainer_seenmask.Trainer(cuda=True, model=m, optimizer=optim.FusedAdam(head, lr=1e-3), train_loader=loader, val_loader=loader,
                                  log_dir=str(tmp_path), dataset="pascal", max_epoch=1, tb_writer=None, checkpoint={}, unseen=UNSEEN,
                                  visualize=2)
    st.validate()
    path = os.path.join(str(tmp_path), "seenmask_viz", "epoch0.jpg")
    assert os.path.exists(path) and Image.open(path).size == (2 * 3 * W, H)
    assert st.last_viz.shape == (H, 2 * 3 * W, 3)
    data, target = next(iter(loader))
    with torch.no_grad():
        _, pred = m.seenmask_predict(data.cuda(), target[0].cuda(), K, UNSEEN)
    want = HV.seenmask(data.numpy(), st.binary_target(target[0]).cpu().numpy(), pred.cpu().numpy(), 1337, np.asarray(loader.dataset.mean_bgr))
    assert np.array_equal(st.last_viz[:, :3 * W], want[0])
