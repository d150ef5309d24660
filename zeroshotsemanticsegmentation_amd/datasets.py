"""datasets.py -- PASCAL-VOC (SBD) and PASCAL-Context-33 readers with the reference's constructor / __getitem__ contract
(/root/reference/pascal_dataset.py:8-146, context_dataset.py:14-160), re-designed around the GPU data path:

  * `native=True` (what train.py uses): __getitem__ returns the RAW sample -- uint8 RGB (H,W,3) image and int64 label
    (H,W) with -1 = ignore.  The BGR / mean subtraction runs on the GPU (utils.image_to_device -> szn_image_u8_to_bgr_f32:
    3 B/px over PCIe instead of 12) and the per-pixel target embedding is gathered on the GPU from the K x E matrix
    (the reference materialises a dense (E,H,W) f32 `lbl_vec` per image on the host: 315 MB at 512x512, E = 300, and
    copies it to the device, trainer_fcn.py:93-95);
  * `native=False`: exactly the reference's outputs -- `transform=True` gives the f32 (3,H,W) BGR-minus-mean image and an
    int64 label, `embed_dim` adds the dense `lbl_vec` as `(lbl, lbl_vec)` -- so existing callers keep working;
  * split filtering (reference: opens EVERY label file at construction, context_dataset.py:75-94, pascal_dataset.py:62-89)
    runs once: the set of classes present in each label file is cached in `<data_dir>/<dataset>/label_presence.json`
    keyed by file size + mtime, and each split is a bit test against it.

Directory layout and split lists are the reference's: `<data_dir>/pascal/benchmark_RELEASE/dataset/{img,cls}`,
`<data_dir>/pascal/VOCdevkit/VOC2012/{JPEGImages,SegmentationClass}`, `<data_dir>/context/33_context_labels`, image ids
from `datasets/<dataset>/<split>.txt` relative to the CWD (override: split_dir=).  Downloading is out of scope (no network).
"""
import json
import os
import os.path as osp

import numpy as np
import torch

from . import utils

MEAN_BGR = np.array(utils.MEAN_BGR)

VOC_CLASSES = ['background', 'aeroplane', 'bicycle', 'bird', 'boat', 'bottle', 'bus', 'car', 'cat', 'chair', 'cow',
               'diningtable', 'dog', 'horse', 'motorbike', 'person', 'potted plant', 'sheep', 'sofa', 'train', 'tv/monitor']
CONTEXT33_CLASSES = ['aeroplane', 'bicycle', 'bird', 'boat', 'bottle', 'bus', 'car', 'cat', 'chair', 'cow', 'diningtable',
                     'dog', 'horse', 'motorbike', 'person', 'pottedplant', 'sheep', 'sofa', 'train', 'tvmonitor', 'sky',
                     'grass', 'ground', 'road', 'building', 'tree', 'water', 'mountain', 'wall', 'floor', 'track',
                     'keyboard', 'ceiling']
INVALID_BIT = 63          # "the label file contains invalid / unlabelled pixels" in the presence mask
# version of everything a cached presence mask depends on besides the file itself: the label decoding rules of the
# _read_label hooks (context: png - 1; voc: 255 -> -1) and the bit layout above.  Bump it when any of them changes: a cache
# written under another version (or for another class list) is discarded, never reused.
PRESENCE_SCHEMA = 2


def _open_image(path):
    import PIL.Image
    return np.array(PIL.Image.open(path), dtype=np.uint8)


def _open_png_label(path):
    import PIL.Image
    return np.array(PIL.Image.open(path), dtype=np.int32)


class _SegmentationDataset(torch.utils.data.Dataset):
    class_names = None
    mean_bgr = MEAN_BGR
    name = None

    def __init__(self, split='train', transform=False, embed_dim=None, one_hot_embed=False, data_dir='data', train_unseen=(),
                 val_unseen=(), native=False, split_dir=None, embed_arr=None, cache=True, hide_unseen=False):
        """hide_unseen (split 'train_seen' only): keep the images the split drops for their unseen classes and hand those classes' pixels
        out as HIDDEN_LABEL instead -- the split then bans only what 'train_seen' bans apart from the unseen classes (_banned_mask)"""
        self.split = split
        self.hide_unseen = bool(hide_unseen)
        if self.hide_unseen and split != 'train_seen':
            raise Exception("hide_unseen belongs to split 'train_seen' (got %r): the other splits show their unseen classes" % (split,))
        self._transform = transform
        self.embed_dim = embed_dim
        self.one_hot_embed = one_hot_embed
        self.data_dir = data_dir
        self.train_unseen = list(train_unseen)
        self.val_unseen = list(val_unseen)
        self.native = native
        if split not in ('train', 'train_seen', 'val'):
            raise Exception("unexpected split for %s dataset" % self.name)
        if (embed_dim or one_hot_embed) and not native:
            self.embed_arr = self._load_embeddings(embed_arr)
        self._cache_path = osp.join(data_dir, self.name, 'label_presence.json') if cache else None
        self._presence = self._load_cache()
        dirty = False
        split_dir = split_dir or osp.join('datasets', self.name)
        split_file = osp.join(split_dir, '%s.txt' % ('train' if split == 'train_seen' else split))
        banned = self._banned_mask()
        self.files = []
        for did in open(split_file):
            did = did.strip()
            if not did:
                continue
            img_file, lbl_file = self._paths(did)
            if banned:
                mask, fresh = self._presence_of(lbl_file)
                dirty |= fresh
                if mask & banned:
                    continue
            self.files.append({'img': img_file, 'lbl': lbl_file})
        if dirty:
            self._save_cache()

    # ---- per-dataset hooks -----------------------------------------------------------------------------------------
    def _paths(self, did):
        raise NotImplementedError

    def _read_label(self, lbl_file):
        """int32 (H,W) in the trainer's numbering: classes 0..K-1, -1 = invalid / ignore"""
        raise NotImplementedError

    def _banned_mask(self):
        raise NotImplementedError

    # ---- split filtering with a presence cache -----------------------------------------------------------------------
    @staticmethod
    def _bits(classes):
        m = 0
        for c in classes:
            m |= 1 << (INVALID_BIT if c < 0 else int(c))
        return m

    def _schema(self):
        import hashlib
        return "%d:%s" % (PRESENCE_SCHEMA, hashlib.sha1("|".join(self.class_names).encode()).hexdigest()[:12])

    def _load_cache(self):
        if self._cache_path and osp.exists(self._cache_path):
            try:
                c = json.load(open(self._cache_path))
            except (OSError, ValueError):
                return {}
            if isinstance(c, dict) and c.get("_schema") == self._schema() and isinstance(c.get("files"), dict):
                return c["files"]
        return {}

    def _save_cache(self):
        if not self._cache_path:
            return
        try:
            os.makedirs(osp.dirname(self._cache_path), exist_ok=True)
            tmp = self._cache_path + '.tmp%d' % os.getpid()
            json.dump({"_schema": self._schema(), "files": self._presence}, open(tmp, 'w'))
            os.replace(tmp, self._cache_path)
        except OSError:
            pass                                      # read-only dataset directory: scan again next time

    def _presence_of(self, lbl_file):
        st = os.stat(lbl_file)
        key = osp.relpath(lbl_file, self.data_dir)
        rec = self._presence.get(key)
        if rec and rec[0] == st.st_size and rec[1] == int(st.st_mtime):
            return rec[2], False
        mask = self._bits(np.unique(self._read_label(lbl_file)).tolist())
        self._presence[key] = [st.st_size, int(st.st_mtime), mask]
        return mask, True

    def class_presence(self, index):
        """the sorted classes that occur in the label of sample `index`, from the presence cache (the label file is opened only where the
        cache has no valid record of it; a fresh record is saved)"""
        mask, fresh = self._presence_of(self.files[index]['lbl'])
        if fresh:
            self._save_cache()
        return [k for k in range(len(self.class_names)) if (mask >> k) & 1]

    # ---- samples -------------------------------------------------------------------------------------------------------
    def _load_embeddings(self, embed_arr):
        if embed_arr is not None:
            return np.asarray(embed_arr, dtype=np.float32)
        if self.one_hot_embed:
            pkl = 'datasets/%s/embeddings/one_hot_%d_dim' % (self.name, len(self.class_names))
            if osp.exists(pkl + '.pkl'):
                return np.asarray(utils.load_obj(pkl), dtype=np.float32)
            return np.eye(len(self.class_names), dtype=np.float32)
        from .trainer_fcn import load_embeddings
        return load_embeddings(self.name, self.embed_dim)

    def __len__(self):
        return len(self.files)

    def __getitem__(self, index):
        f = self.files[index]
        img = _open_image(f['img'])
        lbl = self._read_label(f['lbl'])
        if self.hide_unseen:
            lbl = np.where(np.isin(lbl, self.train_unseen + self.val_unseen), HIDDEN_LABEL, lbl).astype(lbl.dtype)
        if self.native:
            return torch.from_numpy(np.ascontiguousarray(img)), torch.from_numpy(lbl.astype(np.int64))
        lbl_vec = None
        if self.embed_dim:
            idx = np.where(lbl < 0, 0, lbl)                            # row 0 stands in for ignore (and hidden) pixels
            lbl_vec = torch.from_numpy(np.ascontiguousarray(self.embed_arr[idx].transpose(2, 0, 1)))
        if self._transform:
            img, lbl = self.transform(img, lbl)
        return (img, (lbl, lbl_vec)) if self.embed_dim else (img, lbl)

    def transform(self, img, lbl):
        img = img[:, :, ::-1].astype(np.float64) - self.mean_bgr      # RGB -> BGR, minus mean, in float64 like the reference
        img = torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))).float()
        return img, torch.from_numpy(np.ascontiguousarray(lbl)).long()

    def untransform(self, img, lbl):
        img = img.numpy().transpose(1, 2, 0) + self.mean_bgr
        return img.astype(np.uint8)[:, :, ::-1], lbl.numpy() if hasattr(lbl, 'numpy') else lbl


class PascalContext(_SegmentationDataset):
    """33-class PASCAL-Context (context_dataset.py:14-160): label PNGs are 1-based, 0 = unlabelled -> -1 after `lbl - 1`.
    EVERY split drops images that contain unlabelled pixels; 'train' also drops val_unseen classes, 'train_seen' all unseen
    (hide_unseen=True: 'train_seen' keeps them and hides those classes' pixels as HIDDEN_LABEL)."""
    class_names = CONTEXT33_CLASSES
    name = 'context'

    def _paths(self, did):
        return (osp.join(self.data_dir, 'pascal/VOCdevkit/VOC2012', 'JPEGImages/%s.jpg' % did),
                osp.join(self.data_dir, 'context/33_context_labels/%s.png' % did))

    def _read_label(self, lbl_file):
        return _open_png_label(lbl_file) - 1

    def _banned_mask(self):
        extra = {'train': self.val_unseen, 'train_seen': self.train_unseen + self.val_unseen, 'val': []}[self.split]
        return self._bits([-1] + ([] if self.hide_unseen else list(extra)))


class PascalVOC(_SegmentationDataset):
    """21-class PASCAL-VOC: train / train_seen from the SBD .mat files, val from the VOC2012 PNGs, 255 -> -1
    (pascal_dataset.py:8-146).  'train' drops images with val_unseen classes, 'train_seen' with any unseen class, 'val' none.
    (The reference's val branch tests a label left over from the previous loop iteration, pascal_dataset.py:76-89; a val
    split is never filtered here.)"""
    class_names = VOC_CLASSES
    name = 'pascal'

    def _paths(self, did):
        if self.split in ('train', 'train_seen'):
            d = osp.join(self.data_dir, 'pascal/benchmark_RELEASE/dataset')
            return osp.join(d, 'img/%s.jpg' % did), osp.join(d, 'cls/%s.mat' % did)
        d = osp.join(self.data_dir, 'pascal/VOCdevkit/VOC2012')
        return osp.join(d, 'JPEGImages/%s.jpg' % did), osp.join(d, 'SegmentationClass/%s.png' % did)

    def _read_label(self, lbl_file):
        if lbl_file.endswith('.mat'):
            import scipy.io
            lbl = scipy.io.loadmat(lbl_file)['GTcls'][0]['Segmentation'][0].astype(np.int32)
        else:
            lbl = _open_png_label(lbl_file)
        lbl[lbl == 255] = -1
        return lbl

    def _banned_mask(self):
        extra = {'train': self.val_unseen, 'train_seen': self.train_unseen + self.val_unseen, 'val': []}[self.split]
        return self._bits([] if self.hide_unseen else list(extra))


MEAN_RGB_U8 = tuple(int(round(v)) for v in utils.MEAN_BGR[::-1])       # the uint8 colour closest to the mean: ~0 after the transform


PAD_LABEL = -2     # label of the pixels pad_collate adds: ignored by every loss / metric kernel, in BOTH phases (see pad_collate)
# label of the pixels whose unseen class a hide_unseen dataset hides.  Like PAD_LABEL it is below -1, so every existing loss, metric and
# seen-mask kernel ignores it (`target >= 0` in phase 1; szn_seenmask_head and Trainer.binary_target leave labels below -1 out); only
# szn_pseudo_head looks for it (heads.pseudo: the self-training candidates)
HIDDEN_LABEL = -3


def pad_collate(batch):
    """collate_fn for NATIVE samples (uint8 (H,W,3) RGB image, int64 (H,W) label) of different sizes -- PASCAL images differ in
    size (context_dataset.py:143-150 never resizes; the reference therefore trains at batch size 1, train.py:82-84).  Every
    sample is padded at the bottom / right to the largest height / width of the batch: image pixels with the mean colour (zero
    after the BGR - mean transform, i.e. what conv1_1's own zero padding continues with), labels with PAD_LABEL = -2.  Phase 1:
    every loss, class-assignment and histogram kernel ignores negative labels (utils.py:33,60,84: `target >= 0`); per-image losses
    keep their own valid-pixel counts, so a padded batch is the mean of its images' losses.  Phase 2 (trainer_seenmask.py:55-56)
    turns the UNLABELLED value -1 into target 0 = "unseen" and counts it -- padding must not be counted, hence its own value:
    szn_seenmask_head and Trainer.binary_target leave labels below -1 out of the loss, the gradients and the confusion counts.  -> ((B,Hm,Wm,3) uint8, (B,Hm,Wm)
    int64).  Samples that carry the reference's (label, label_embedding) tuple keep the label only (the embedding is gathered
    on the GPU)."""
    imgs, lbls = [], []
    for img, lbl in batch:
        if isinstance(lbl, (tuple, list)):
            lbl = lbl[0]
        img, lbl = torch.as_tensor(img), torch.as_tensor(lbl)
        if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
            raise ValueError("pad_collate expects native samples: uint8 (H,W,3) images (datasets built with native=True)")
        imgs.append(img)
        lbls.append(lbl.long())
    Hm, Wm = max(i.shape[0] for i in imgs), max(i.shape[1] for i in imgs)
    out_i = torch.empty(len(imgs), Hm, Wm, 3, dtype=torch.uint8)
    out_i[:] = torch.tensor(MEAN_RGB_U8, dtype=torch.uint8)
    out_l = torch.full((len(imgs), Hm, Wm), PAD_LABEL, dtype=torch.int64)
    for k, (img, lbl) in enumerate(zip(imgs, lbls)):
        h, w = img.shape[:2]
        out_i[k, :h, :w] = img
        out_l[k, :h, :w] = lbl
    return out_i, out_l


def augment_collate(batch):
    """pad_collate for the augmented training route (train.py --crop-size): the same padded (B,Hm,Wm,3) uint8 canvases and (B,Hm,Wm)
    int64 labels, plus the images' own sizes as a THIRD element, int32 (B,2) = (h, w) -- what Augment.params scales and the kernel needs to
    keep the canvas padding out of its bilinear taps.  A trainer built with augment= unpacks three elements; the padded pair is never
    shown to the network as it is."""
    sizes = torch.tensor([tuple(torch.as_tensor(img).shape[:2]) for img, _ in batch], dtype=torch.int32).reshape(len(batch), 2)
    out_i, out_l = pad_collate(batch)
    return out_i, out_l, sizes


class Augment(object):
    """Random scale, crop to a fixed size and horizontal flip per training image (utils.augment_to_device / szn_augment_u8 do the
    pixels; this class only draws the numbers).  crop = (H, W) of the network input; scale = (lo, hi): one isotropic s ~ U[lo, hi] per
    image; flip: mirror with probability 1/2.  Where the scaled image is larger than the crop the window origin is uniform over
    [0, Hs - H] x [0, Ws - W]; where it is smaller the origin is 0: the image sits top-left and PAD_LABEL padding fills the bottom and
    right, as pad_collate pads.  Every draw is a pure function of (seed, rank, epoch, iteration, index in the batch) -- a Philox
    counter-based generator keyed by (seed, rank) at counter (epoch, iteration, index) -- so a resumed run and every rank of a
    data-parallel job reproduce their own stream, and ranks differ.

    rotate = R >= 0 degrees and jitter = dict(brightness=B, contrast=C, saturation=S, hue=Hdeg), each >= 0, add a rotation by
    phi ~ U[-R, R] about the image centre and a photometric chain -- brightness x + 255 b, b ~ U[-B, B]; contrast about the mean colour,
    alpha ~ U[1-C, 1+C]; saturation about the luma, sigma ~ U[1-S, 1+S]; hue, a rotation by theta ~ U[-Hdeg, Hdeg] about the grey axis --
    each applied at its drawn strength to every image (no coin flips; a zero range switches a transform off exactly).  With either set,
    params() returns the 20-word affine record of szn_augment_affine_u8 and apply() launches that kernel; with rotate == 0 and jitter
    None both do exactly what they did before.  The first four numbers of an image's draw are the same in both modes, so its scale,
    window draw and mirror do not depend on the options."""

    JITTER_KEYS = ("brightness", "contrast", "saturation", "hue")
    LUMA = (0.299, 0.587, 0.114)

    def __init__(self, crop, scale=(0.5, 2.0), flip=True, seed=1337, rotate=0.0, jitter=None):
        self.crop = (int(crop[0]), int(crop[1]))
        self.scale = (float(scale[0]), float(scale[1]))
        self.flip = bool(flip)
        self.seed = int(seed)
        if self.crop[0] < 1 or self.crop[1] < 1:
            raise ValueError("Augment: crop %s must be positive" % (self.crop,))
        if not 0.0 < self.scale[0] <= self.scale[1]:
            raise ValueError("Augment: scale range %s must satisfy 0 < lo <= hi" % (self.scale,))
        self.rotate = float(rotate)
        if not 0.0 <= self.rotate < float("inf"):
            raise ValueError("Augment: rotate %r must be a finite angle >= 0 (degrees)" % (rotate,))
        self.jitter = None
        if jitter is not None:
            unknown = sorted(set(jitter) - set(self.JITTER_KEYS))
            if unknown:
                raise ValueError("Augment: jitter knows %s, not %s" % (", ".join(self.JITTER_KEYS), unknown))
            self.jitter = tuple(float(jitter.get(k, 0.0)) for k in self.JITTER_KEYS)
            if not all(0.0 <= v < float("inf") for v in self.jitter):
                raise ValueError("Augment: jitter strengths %s must be finite and >= 0" % (dict(zip(self.JITTER_KEYS, self.jitter)),))
        self.affine = self.rotate != 0.0 or self.jitter is not None

    @staticmethod
    def record(h, w, s, oy_u=0.0, ox_u=0.0, flip=False, crop=None):
        """the int32 record of one image (include/szn.h): scaled size Hs = max(1, floor(h*s + 0.5)), 16.16 step ((h << 16) + Hs/2) / Hs,
        window origin floor(u * (Hs - H + 1)) for u in [0, 1) where the scaled image exceeds the crop (H, W), else 0"""
        h, w = int(h), int(w)
        Hs, Ws = max(1, int(np.floor(h * s + 0.5))), max(1, int(np.floor(w * s + 0.5)))
        if max(h, w, Hs, Ws) >= 1 << 15:
            raise ValueError("Augment: image %d x %d scaled to %d x %d exceeds the 16.16 fixed-point range" % (h, w, Hs, Ws))
        oy = min(int(oy_u * (Hs - crop[0] + 1)), Hs - crop[0]) if crop is not None and Hs > crop[0] else 0
        ox = min(int(ox_u * (Ws - crop[1] + 1)), Ws - crop[1]) if crop is not None and Ws > crop[1] else 0
        return [h, w, Hs, Ws, ((h << 16) + Hs // 2) // Hs, ((w << 16) + Ws // 2) // Ws, oy, ox, int(bool(flip))]

    @staticmethod
    def bridge(rec, crop):
        """the 9-word record of szn_augment_u8 as the 8 geometry words of szn_augment_affine_u8 (include/szn.h, axis-aligned identity):
        the same source positions, exactly"""
        h, w, _, _, step_y, step_x, oy, ox, flip = [int(v) for v in rec]
        return [h, w, -step_x if flip else step_x, 0, step_x * (ox + (int(crop[1]) if flip else 0)), 0, step_y, step_y * oy]

    @staticmethod
    def color_matrix(b=0.0, alpha=1.0, sigma=1.0, theta=0.0, mean_bgr=utils.MEAN_BGR):
        """the photometric chain as one affine map of RGB grey levels, float64: brightness x + 255 b; contrast m + alpha (x - m) about the
        mean colour m; saturation g + sigma (x - g), g = the luma 0.299 R + 0.587 G + 0.114 B; hue, the rotation by theta degrees about
        the grey axis (1,1,1) -> (M (3,3), o (3,)) with x_out = M x + o.  b = 0, alpha = sigma = 1, theta = 0 give exactly (I, 0)."""
        m = np.asarray(mean_bgr, dtype=np.float64)[::-1]
        one = np.ones(3)
        S = sigma * np.eye(3) + (1.0 - sigma) * np.outer(one, np.asarray(Augment.LUMA))
        t = np.deg2rad(theta)
        K = np.array([[0.0, -1.0, 1.0], [1.0, 0.0, -1.0], [-1.0, 1.0, 0.0]])
        R = np.cos(t) * np.eye(3) + (1.0 - np.cos(t)) / 3.0 * np.outer(one, one) + np.sin(t) / np.sqrt(3.0) * K
        RS = R @ S
        return alpha * RS, RS @ (alpha * 255.0 * b * one + (1.0 - alpha) * m)

    @staticmethod
    def color_words(M, o):
        """(M, o) of color_matrix -> the 12 Q16 words Cm (row-major), Co of the record; a matrix entry beyond +-16 (the kernel's clamp of
        +-2^20) or an offset beyond the int32 range is refused"""
        cm = np.rint(65536.0 * np.asarray(M, dtype=np.float64)).reshape(9)
        co = np.rint(65536.0 * np.asarray(o, dtype=np.float64)).reshape(3)
        if not (np.all(np.isfinite(cm)) and np.all(np.isfinite(co))) or np.abs(cm).max() > 1 << 20 or np.abs(co).max() >= 1 << 31:
            raise ValueError("Augment: colour matrix %s, offset %s outside the Q16 range of the record" % (np.asarray(M).tolist(), np.asarray(o).tolist()))
        return [int(v) for v in cm] + [int(v) for v in co]

    @staticmethod
    def affine_record(h, w, s, phi=0.0, oy_u=0.0, ox_u=0.0, flip=False, crop=None, color=None):
        """the 20-word int32 record of one image (szn_augment_affine_u8, include/szn.h).  The image is scaled to record()'s Hs x Ws and
        rotated by phi degrees about its centre; the rotated image sits centred in its bounding box Wb = |cos| Ws + |sin| Hs,
        Hb = |sin| Ws + |cos| Hs; the crop window's origin is u * (Hb - H) for u in [0, 1) where the box exceeds the crop (H, W), else
        0; the mirror comes last.  The inverse map (output pixel -> source position) is composed in float64 and rounded once to 16.16.
        phi == 0 takes the bridge of record() instead: exactly the positions of szn_augment_u8.  color = (M, o) of color_matrix, None =
        the identity.  Two choices differ from the textbook form Rinv / s with an integer window: the inverse scale is
        diag(w / Ws, h / Hs), the ratios of the ROUNDED sizes, so that the scaled image is exactly Hs x Ws and phi -> 0 meets the bridge;
        and the window origin over the box is real-valued, because the box's sides are."""
        h, w = int(h), int(w)
        if flip and crop is None:
            raise ValueError("Augment: the mirror is taken about the crop's centre line: flip needs crop=(H, W)")
        rec9 = Augment.record(h, w, s, oy_u, ox_u, flip, crop)
        Hs, Ws = rec9[2], rec9[3]
        if max(h, w, Hs, Ws) >= 1 << 14:
            raise ValueError("Augment: image %d x %d scaled to %d x %d exceeds the 16.16 fixed-point range of the affine record" % (h, w, Hs, Ws))
        if phi == 0.0:
            geo = Augment.bridge(rec9, crop if crop is not None else (0, 0))
        else:
            c, sn = np.cos(np.deg2rad(phi)), np.sin(np.deg2rad(phi))
            c, sn = (0.0 if abs(c) < 1e-15 else c), (0.0 if abs(sn) < 1e-15 else sn)      # quarter turns are exact
            Wb, Hb = abs(c) * Ws + abs(sn) * Hs, abs(sn) * Ws + abs(c) * Hs
            Hc, Wc = (crop if crop is not None else (0, 0))
            oy = oy_u * (Hb - Hc) if crop is not None and Hb > Hc else 0.0
            ox = ox_u * (Wb - Wc) if crop is not None and Wb > Wc else 0.0
            # source pixels per pixel of the scaled image, per axis (the rounded sizes, as in record()), times the inverse rotation
            ax, ay = w / Ws, h / Hs
            A = np.array([[ax * c, ax * sn], [-ay * sn, ay * c]])
            org = np.array([ox + (Wc if flip else 0) - Wb / 2.0, oy - Hb / 2.0])
            t = A @ org + np.array([w / 2.0, h / 2.0])
            if flip:
                A[:, 0] = -A[:, 0]
            geo = [h, w] + [int(v) for v in np.rint(65536.0 * np.array([A[0, 0], A[0, 1], t[0], A[1, 0], A[1, 1], t[1]]))]
        if max(abs(v) for v in geo) >= 1 << 31:
            raise ValueError("Augment: the affine map %s of image %d x %d leaves the int32 16.16 range" % (geo[2:], h, w))
        return geo + (Augment.color_words(*color) if color is not None else [65536, 0, 0, 0, 65536, 0, 0, 0, 65536, 0, 0, 0])

    def draw(self, i, epoch, iteration, rank=0):
        """image i's nine uniform numbers: scale, window y, window x, mirror, then rotation, brightness, contrast, saturation, hue"""
        bits = np.random.Philox(key=[self.seed, int(rank)], counter=[int(epoch), int(iteration), i, 0])
        return np.random.Generator(bits).random(9 if self.affine else 4)

    def params(self, sizes, epoch, iteration, rank=0, mean_bgr=utils.MEAN_BGR):
        """sizes (B,2) = (h, w) per image -> int32 numpy (B, AUG_NPARAM), or (B, AUGA_NPARAM) with rotate / jitter set (mean_bgr is the
        pivot of the contrast and only read then)"""
        sizes = np.asarray(sizes).reshape(-1, 2)
        out = np.empty((len(sizes), utils.L.AUGA_NPARAM if self.affine else utils.L.AUG_NPARAM), dtype=np.int32)
        lo, hi = self.scale
        jb, jc, js, jh = self.jitter or (0.0, 0.0, 0.0, 0.0)
        for i, (h, w) in enumerate(sizes):
            u = self.draw(i, epoch, iteration, rank)
            s, flip = lo + (hi - lo) * u[0], self.flip and u[3] < 0.5
            if not self.affine:
                out[i] = self.record(h, w, s, u[1], u[2], flip, self.crop)
                continue
            d = 2.0 * u[4:9] - 1.0                                                       # U[-1, 1)
            color = self.color_matrix(jb * d[1], 1.0 + jc * d[2], 1.0 + js * d[3], jh * d[4], mean_bgr)
            out[i] = self.affine_record(h, w, s, self.rotate * d[0], u[1], u[2], flip, self.crop, color)
        return out

    def apply(self, batch, epoch, iteration, rank=0, device=None, mean_bgr=utils.MEAN_BGR):
        """one augment_collate batch (images, labels, sizes) -> (data (B,3,H,W) f32, target (B,H,W) int64) on the device"""
        if not isinstance(batch, (tuple, list)) or len(batch) != 3:
            raise ValueError("Augment needs (images, labels, sizes) batches: build the training loaders with collate_fn=datasets.augment_collate")
        img, lbl, sizes = batch
        if self.affine:
            return utils.augment_affine_to_device(img, lbl, self.params(sizes, epoch, iteration, rank, mean_bgr), self.crop, device, mean_bgr)
        return utils.augment_to_device(img, lbl, self.params(sizes, epoch, iteration, rank), self.crop, device, mean_bgr)


class SupportSet(torch.utils.data.Dataset):
    """The strict K-shot support set of few-shot prototype adaptation (SPNet's few-label protocol): for each class of `classes`, in
    ascending order, the first `shots` samples of `base`, in ascending index, whose label holds at least one pixel of it.  Items are
    (base index, class) pairs (`items`); item i is base's sample with the label reduced to where(lbl == class, class, -1): a shot
    reveals one class's mask and nothing else.  `base` must show the classes: a real dataset's split 'train' built with empty unseen
    lists (class presence then comes from its presence cache, class_presence), SyntheticSegmentation(split='train', unseen=[]) (from
    the generated label).  `found` maps each class to the number of shots it got (fewer than `shots` where base runs out)."""

    def __init__(self, base, classes, shots):
        self.base = base
        self.classes = sorted(set(int(k) for k in classes))
        self.shots = int(shots)
        if self.shots < 1:
            raise ValueError("SupportSet: shots must be at least 1, got %r" % (shots,))
        if not self.classes or self.classes[0] < 0:
            raise ValueError("SupportSet: classes must name at least one class index >= 0, got %r" % (classes,))
        want = set(self.classes)
        per_class = {k: [] for k in self.classes}
        for index in range(len(base)):
            if all(len(v) >= self.shots for v in per_class.values()):
                break
            for k in sorted(want & set(self._present(index))):
                if len(per_class[k]) < self.shots:
                    per_class[k].append(index)
        self.items = [(index, k) for k in self.classes for index in per_class[k]]
        self.found = {k: len(per_class[k]) for k in self.classes}

    def _present(self, index):
        if hasattr(self.base, 'class_presence'):
            return self.base.class_presence(index)
        lbl = self._label_of(self.base[index])
        return [int(k) for k in np.unique(np.asarray(lbl)) if k >= 0]

    @staticmethod
    def _label_of(sample):
        lbl = sample[1]
        return lbl[0] if isinstance(lbl, (tuple, list)) else lbl

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        index, k = self.items[i]
        sample = self.base[index]
        lbl = self._label_of(sample)
        if isinstance(lbl, torch.Tensor):
            one = torch.where(lbl == k, lbl, torch.full_like(lbl, -1))
        else:
            lbl = np.asarray(lbl)
            one = np.where(lbl == k, lbl, -1).astype(lbl.dtype)
        rest = sample[1]
        new_lbl = (one,) + tuple(rest[1:]) if isinstance(rest, (tuple, list)) else one
        return (sample[0], new_lbl) + tuple(sample[2:])


def download(data_dir):
    """the reference fetches SBD / VOC2012 / the 33-class context labels over HTTP (pascal_dataset.py:148-172,
    context_dataset.py:162-183); this environment has no network, so the data must already be under data_dir"""
    raise IOError("no network access: place the datasets under %s (layout in the module docstring)" % data_dir)
