"""vis_utils.py -- validation visualisations, rendered on the GPU.

Mirrors the reference's vis_utils.py (visualize_seenmask :4-31, visualize_segmentation :34-109, make_seen_mask :111-116): per image the
input, the colourised truth and prediction, their overlay on the grey image and the seen / unseen mask, tiled into one picture.  The
reference draws on the host through the third-party `fcn` package; here one HIP kernel (csrc/szn_viz.hip, contract in include/szn.h)
writes the finished uint8 panels from device tensors.  There is no CPU drawing path.

  visualize_segmentation / visualize_seenmask / make_seen_mask     the reference's names: numpy in, numpy out (upload, kernel, download)
  visualize_segmentation_device / visualize_seenmask_device        device tensors in, device tensor out (what the trainers call)
  get_tile_image                                                   the mosaic of a list of device visualisations
  label_colormap                                                   the class colours on the host (legends, tests)

Stated differences from the reference: the network input is un-transformed by rounding, not truncation (exact for every byte);
unlabelled pixels are -1 AND anything outside [0, n_class) (the batch padding -2), filled with seeded noise (the reference's is
unseeded); no legend is drawn (`label_names` is accepted and ignored); the mosaic centres tiles on black and resamples nothing.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L
from .utils import MEAN_BGR


def label_colormap(n=256):
    """(n, 3) uint8: the PASCAL bit-shuffle colour map the kernel computes per pixel (class 1 -> (128, 0, 0), 15 -> (192, 128, 128))"""
    cmap = np.zeros((n, 3), dtype=np.uint8)
    for k in range(n):
        c, r, g, b = k, 0, 0, 0
        for j in range(8):
            r |= (c & 1) << (7 - j)
            g |= ((c >> 1) & 1) << (7 - j)
            b |= ((c >> 2) & 1) << (7 - j)
            c >>= 3
        cmap[k] = (r, g, b)
    return cmap


def _image_arg(data):
    """-> (contiguous device tensor, img_kind, B, H, W): uint8 RGB (B,H,W,3) = kind 0, the f32 network input (B,3,H,W) = kind 1"""
    if not isinstance(data, torch.Tensor) or not data.is_cuda:
        raise L.SznError("the image must be a GPU tensor (the HIP path has no CPU fallback)")
    if data.dtype == torch.uint8 and data.dim() == 4 and data.shape[3] == 3:
        return data.contiguous(), 0, data.shape[0], data.shape[1], data.shape[2]
    if data.dtype == torch.float32 and data.dim() == 4 and data.shape[1] == 3:
        return data.contiguous(), 1, data.shape[0], data.shape[2], data.shape[3]
    raise L.SznError("the image must be uint8 (B,H,W,3) or float32 (B,3,H,W), got %s %s" % (data.dtype, tuple(data.shape)))


def _label_arg(lbl, B, H, W, what, dev):
    if lbl is None:
        return None
    if tuple(lbl.shape) != (B, H, W):
        raise L.SznError("%s must be (%d, %d, %d), got %s" % (what, B, H, W, tuple(lbl.shape)))
    return lbl.to(device=dev, dtype=torch.int64).contiguous()


def _out_arg(out, shape, dev):
    """the output tensor and its (row, image) byte strides: a fresh dense tensor, or the caller's view into a larger uint8 canvas"""
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=dev)
    if (out.dtype != torch.uint8 or tuple(out.shape) != tuple(shape) or out.device != dev or out.stride(3) != 1
            or out.stride(2) != 3):
        raise L.SznError("out must be a uint8 %s view on %s with dense pixels" % (tuple(shape), dev))
    return out, out.stride(1), out.stride(0)


def visualize_segmentation_device(data, lbl_true, lbl_pred, n_class, unseen=None, seed=1337, out=None, mean_bgr=MEAN_BGR):
    """data (B,H,W,3) uint8 RGB or (B,3,H,W) f32 network input, lbl_true (B,H,W) or None, lbl_pred (B,H,W), all on the device ->
    (B, rows*H, n_col*W, 3) uint8 device tensor: rows = truth, prediction (prediction only without lbl_true), columns = image | class
    colours | overlay on grey | seen mask (the last only with a non-empty `unseen`).  One launch, no host synchronisation."""
    return _segmentation(data, lbl_true, lbl_pred, n_class, L.class_set(unseen), seed, out, mean_bgr)


def _segmentation(data, lbl_true, lbl_pred, n_class, cs, seed=1337, out=None, mean_bgr=MEAN_BGR):
    """cs: a _lib.class_set argument; None = no mask column"""
    img, kind, B, H, W = _image_arg(data)
    lt = _label_arg(lbl_true, B, H, W, "lbl_true", img.device)
    lp = _label_arg(lbl_pred, B, H, W, "lbl_pred", img.device)
    if lp is None:
        raise ValueError('lbl_pred must be not None.')
    rows, n_col = (2 if lt is not None else 1), (4 if cs is not None else 3)
    out, row_bytes, image_bytes = _out_arg(out, (B, rows * H, n_col * W, 3), img.device)
    mean = (C.c_double * 3)(*[float(m) for m in mean_bgr])
    L.call("szn_viz_segmentation", B, H, W, L.ptr(img), kind, mean, L.ptr(lt), L.ptr(lp), int(n_class), cs, int(seed), L.ptr(out),
           row_bytes, image_bytes, L.stream_ptr())
    return out


def visualize_seenmask_device(data, lbl_true, lbl_pred, seed=1337, out=None, mean_bgr=MEAN_BGR):
    """the seen-mask layout: (B, H, 3*W, 3) uint8 = image | 255 * (lbl_true == 1) | 255 * (lbl_pred == 1); lbl_true < 0 is noise"""
    img, kind, B, H, W = _image_arg(data)
    lt = _label_arg(lbl_true, B, H, W, "lbl_true", img.device)
    lp = _label_arg(lbl_pred, B, H, W, "lbl_pred", img.device)
    if lt is None or lp is None:
        raise ValueError('lbl_true and lbl_pred must be not None.')
    out, row_bytes, image_bytes = _out_arg(out, (B, H, 3 * W, 3), img.device)
    mean = (C.c_double * 3)(*[float(m) for m in mean_bgr])
    L.call("szn_viz_seenmask", B, H, W, L.ptr(img), kind, mean, L.ptr(lt), L.ptr(lp), int(seed), L.ptr(out), row_bytes, image_bytes,
           L.stream_ptr())
    return out


def mosaic_shape(n):
    """(rows, columns) of a mosaic of n pictures: floor(sqrt(n)) rows, as many columns as that takes (25 -> 5 x 5)"""
    rows = max(math.isqrt(n), 1)
    return rows, int(math.ceil(n / float(rows)))


def get_tile_image(vizs, tile_shape=None):
    """list of (h_i, w_i, 3) uint8 device tensors -> one (rows*cell_h, cols*cell_w, 3) uint8 device tensor.  Every cell has the largest
    height and width in the list; each picture is centred in its cell on black.  Nothing is resampled (`fcn` rescales)."""
    if not vizs:
        raise ValueError("get_tile_image needs at least one picture")
    rows, cols = tile_shape if tile_shape is not None else mosaic_shape(len(vizs))
    if rows * cols < len(vizs):
        raise ValueError("tile_shape %s holds fewer than %d pictures" % ((rows, cols), len(vizs)))
    ch, cw = max(v.shape[0] for v in vizs), max(v.shape[1] for v in vizs)
    canvas = torch.zeros(rows * ch, cols * cw, 3, dtype=torch.uint8, device=vizs[0].device)
    for i, v in enumerate(vizs):
        y = (i // cols) * ch + (ch - v.shape[0]) // 2
        x = (i % cols) * cw + (cw - v.shape[1]) // 2
        canvas[y:y + v.shape[0], x:x + v.shape[1]] = v
    return canvas


# ---- the reference's names: numpy in, numpy out -----------------------------------------------------------------------------------
def _to_device(img, *lbls):
    dev = torch.device("cuda", torch.cuda.current_device())
    img = np.ascontiguousarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise L.SznError("img must be a uint8 (H,W,3) RGB array, got %s %s" % (img.dtype, img.shape))
    up = lambda a: None if a is None else torch.from_numpy(np.array(a, dtype=np.int64)).unsqueeze(0).to(dev)   # a copy: the caller's stays
    return [torch.from_numpy(img).unsqueeze(0).to(dev)] + [up(a) for a in lbls]


def visualize_segmentation(**kwargs):
    """img (H,W,3) uint8 RGB, lbl_true (H,W) (or None: prediction row only), lbl_pred (H,W), n_class, unseen, label_names -> the
    (2H, n_col*W, 3) uint8 picture of reference vis_utils.py:34-109.  `label_names` is accepted and ignored: the legend `fcn` draws
    with matplotlib is not reproduced.  The caller's label arrays are not modified (the reference zeroes lbl_true in place)."""
    img = kwargs.pop('img', None)
    lbl_true = kwargs.pop('lbl_true', None)
    lbl_pred = kwargs.pop('lbl_pred', None)
    n_class = kwargs.pop('n_class', None)
    kwargs.pop('label_names', None)
    unseen = kwargs.pop('unseen', None)
    if kwargs:
        raise RuntimeError('Unexpected keys in kwargs: {}'.format(kwargs.keys()))
    if lbl_pred is None:
        raise ValueError('lbl_pred must be not None.')
    img, lt, lp = _to_device(img, lbl_true, lbl_pred)
    return visualize_segmentation_device(img, lt, lp, n_class, unseen)[0].cpu().numpy()


def visualize_seenmask(**kwargs):
    """img, lbl_true, lbl_pred (binary: 1 = seen), unseen, n_class -> the (H, 3W, 3) uint8 picture of reference vis_utils.py:4-31
    (`unseen` and `n_class` are accepted and unused, as there)"""
    img = kwargs.pop('img', None)
    lbl_true = kwargs.pop('lbl_true', None)
    lbl_pred = kwargs.pop('lbl_pred', None)
    kwargs.pop('unseen', None)
    kwargs.pop('n_class', None)
    if kwargs:
        raise RuntimeError('Unexpected keys in kwargs: {}'.format(kwargs.keys()))
    if lbl_true is None or lbl_pred is None:
        raise ValueError('lbl_true and lbl_pred must be not None.')
    img, lt, lp = _to_device(img, lbl_true, lbl_pred)
    return visualize_seenmask_device(img, lt, lp)[0].cpu().numpy()


def make_seen_mask(lbl, unseen, n_class):
    """(H,W) labels -> (H,W,3) uint8, 255 where the label is a seen class (reference :111-116).  Rendered by the same kernel: the mask
    panel of a prediction-only segmentation picture."""
    lbl = np.asarray(lbl)
    H, W = lbl.shape
    dev = torch.device("cuda", torch.cuda.current_device())
    lp = torch.from_numpy(np.array(lbl, dtype=np.int64)).unsqueeze(0).to(dev)
    img = torch.zeros(1, H, W, 3, dtype=torch.uint8, device=dev)
    cs = L.class_set(unseen) or C.byref(L.ClassSet())          # an empty set still asks for the mask column
    return _segmentation(img, None, lp, n_class, cs)[0, :, 3 * W:].cpu().numpy().copy()


# ---- the trainers' per-epoch picture ----------------------------------------------------------------------------------------------
def dataset_mean_bgr(dataset):
    """the mean the dataset's transform subtracted (through torch.utils.data.Subset wrappers); the datasets' common default otherwise"""
    while not hasattr(dataset, 'mean_bgr') and hasattr(dataset, 'dataset'):
        dataset = dataset.dataset
    return tuple(float(m) for m in getattr(dataset, 'mean_bgr', MEAN_BGR))


def save_mosaic(tiles, path):
    """tiles (list of device pictures) -> mosaic as numpy (one device-to-host copy), written to `path` as JPEG"""
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError("--viz (Trainer(visualize=N)) writes JPEG files through PIL, which cannot be imported: %s" % e)
    mosaic = get_tile_image(tiles).cpu().numpy()
    Image.fromarray(mosaic).save(path)
    return mosaic
