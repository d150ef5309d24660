"""numpy int64 restatement of the augmentation contract of szn_augment_u8 (include/szn.h) and of the host side of its per-image record,
written from the text of the contract, not from the kernel.  tests/test_augment_ref.py pins it to independent anchors (the dataset
transform, np.flip, exact 2x2 means, torch's bilinear interpolation); tests/test_gpu_augment.py demands bit equality of the kernel.

The record (int32 x NPARAM): h, w, Hs, Ws, step_y, step_x, oy, ox, flip.

Distance from real-valued bilinear interpolation (`interp_bound`).  The integer arithmetic itself is exact (v <= 255 * 2^22 fits int32), so
the result IS the continuous bilinear interpolant f of the byte image, evaluated at a slightly different position (y', x') than the exact
pixel-centre position y = (gy + 1/2) * h / Hs - 1/2 (clamped to [0, h-1]; clamping never increases a distance):
  * the step is h * 2^16 / Hs rounded to an integer: off by at most 1/2 unit of 2^-16 px.  It is multiplied by (2*gy + 1) / 2 <= Hs - 1/2,
    so the position drifts by less than Hs * 2^-17 px over the image;
  * the `>> 1` of the product drops at most 1/2 unit: 2^-17 px;
  * the weight keeps 11 of the 16 fraction bits: y' is below the fixed-point position by less than 2^-11 px.
So |y' - y| < e(Hs) = 2^-11 + (Hs + 1) * 2^-17, and |x' - x| < e(Ws).  f is piecewise linear and continuous along each axis with a slope of
at most 255 per pixel (neighbouring bytes differ by at most 255), hence
    |v / 2^22 - f(y, x)| < 255 * (e(Hs) + e(Ws)).
torch's own float64 rounding (~1e-13) is far below the last digit of that bound and is not added.
"""
import numpy as np

NPARAM = 9
PAD_LABEL = -2
MEAN_BGR = (104.00698793, 116.66876762, 122.67891434)


def record(h, w, s, oy=0, ox=0, flip=False):
    """the host side of the record: Hs = max(1, floor(h*s + 0.5)), step_y = ((h << 16) + Hs/2) / Hs, the same in x"""
    h, w = int(h), int(w)
    Hs = max(1, int(np.floor(h * s + 0.5)))
    Ws = max(1, int(np.floor(w * s + 0.5)))
    return [h, w, Hs, Ws, ((h << 16) + Hs // 2) // Hs, ((w << 16) + Ws // 2) // Ws, int(oy), int(ox), int(bool(flip))]


def _axis(g, step, n):
    """grid coordinates g (int64, inside the scaled image) -> taps i0, i1, the 11-bit weight of i1, the nearest index of the label"""
    s = (((2 * g + 1) * np.int64(step)) >> 1) - 32768
    sc = np.clip(s, 0, np.int64(n - 1) << 16)
    i0 = sc >> 16
    i1 = np.minimum(i0 + 1, n - 1)
    wgt = (sc & 0xffff) >> 5
    near = np.clip((s + 32768) >> 16, 0, n - 1)
    return i0, i1, wgt, near


def fixed_point(img, label, rec, out_hw):
    """one image: uint8 canvas (Hm,Wm,3), label (Hm,Wm), record -> (v int64 (Ho,Wo,3) RGB order = value * 2^22, label int64 (Ho,Wo),
    pad bool (Ho,Wo)); v is 0 where pad"""
    h, w, Hs, Ws, step_y, step_x, oy, ox, flip = [int(r) for r in rec]
    Ho, Wo = out_hw
    yo = np.arange(Ho, dtype=np.int64)
    xo = np.arange(Wo, dtype=np.int64)
    gy = yo + oy
    gx = (Wo - 1 - xo if flip else xo) + ox
    in_y, in_x = (gy >= 0) & (gy < Hs), (gx >= 0) & (gx < Ws)
    pad = ~(in_y[:, None] & in_x[None, :])
    y0, y1, wy, ly = _axis(np.where(in_y, gy, 0), step_y, h)
    x0, x1, wx, lx = _axis(np.where(in_x, gx, 0), step_x, w)
    p = np.asarray(img).astype(np.int64)
    wy, wx = wy[:, None, None], wx[None, :, None]
    top = (2048 - wx) * p[y0][:, x0] + wx * p[y0][:, x1]
    bot = (2048 - wx) * p[y1][:, x0] + wx * p[y1][:, x1]
    v = (2048 - wy) * top + wy * bot
    assert v.max() <= 255 << 22 and v.min() >= 0
    v[pad] = 0
    lab = np.asarray(label).astype(np.int64)[ly][:, lx]
    lab[pad] = PAD_LABEL
    return v, lab, pad


def augment(img, label, params, out_hw, mean_bgr=MEAN_BGR):
    """the batch: uint8 (B,Hm,Wm,3), labels (B,Hm,Wm), records (B,NPARAM) -> (float32 (B,3,Ho,Wo) BGR minus mean, int64 (B,Ho,Wo));
    padding is exactly 0.0 / PAD_LABEL"""
    B = len(img)
    Ho, Wo = out_hw
    data = np.zeros((B, 3, Ho, Wo), dtype=np.float32)
    target = np.empty((B, Ho, Wo), dtype=np.int64)
    mean = np.asarray(mean_bgr, dtype=np.float64)
    for b in range(B):
        v, lab, pad = fixed_point(img[b], label[b], params[b], out_hw)
        bgr = (v[:, :, ::-1].astype(np.float64) / 4194304.0 - mean).astype(np.float32)
        bgr[pad] = 0.0
        data[b] = bgr.transpose(2, 0, 1)
        target[b] = lab
    return data, target


def interp_bound(Hs, Ws):
    """upper bound of |v / 2^22 - exact bilinear interpolation| (module docstring)"""
    e = lambda n: 2.0 ** -11 + (n + 1) * 2.0 ** -17
    return 255.0 * (e(Hs) + e(Ws))
