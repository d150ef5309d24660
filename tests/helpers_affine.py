"""numpy int64 restatement of the contract of szn_augment_affine_u8 (include/szn.h): a 2 x 3 fixed-point affine position map and a 3 x 4
fixed-point colour matrix per image -- written from the text of the contract, not from the kernel.  tests/test_affine_ref.py pins it to
independent anchors (helpers_augment's restatement of szn_augment_u8 through the bridge record, np.rot90, an exact float64 bilinear
interpolation, a sequential float64 photometric chain); tests/test_gpu_affine.py demands bit equality of the kernel.

The record (int32 x NPARAM): h, w, mxx, mxy, tx, myx, myy, ty, Cm[3][3] (row-major, RGB in, RGB out, Q16), Co[3] (grey levels, Q16).

The host geometry is restated here too (`affine_float`): the image is scaled to helpers_augment.record's Hs x Ws, rotated by phi about its
centre, centred in its bounding box Wb = |cos| Ws + |sin| Hs, Hb = |sin| Ws + |cos| Hs; a crop window at (oy, ox) of the box; the mirror
last.  With continuous coordinates in which pixel i covers [i, i + 1), output pixel (yo, xo) has the centre (xo + 1/2, yo + 1/2), the
window moves it to (xo' + 1/2 + ox, yo + 1/2 + oy) in the box (xo' = Wo - 1 - xo under the mirror), and the source point is
    p = D Rinv ((u, v) - (Wb/2, Hb/2)) + (w/2, h/2),     Rinv = [[cos, sin], [-sin, cos]],   D = diag(w / Ws, h / Hs),
the sample position in index space p - 1/2.  The contract's sx / 65536 = mxx (xo + 1/2) + mxy (yo + 1/2) + tx - 1/2 is that map.

Distance from real-valued bilinear interpolation (`interp_bound`).  The integer interpolation is exact (acc <= 255 * 2^22), so acc / 2^22 IS
the continuous bilinear interpolant f of the byte image, evaluated at a position (y', x') slightly off the exact affine position (y, x)
(both clamped to the image; clamping never increases a distance).  Along x, in pixels:
  * mxx is the real coefficient times 2^16 rounded to an integer, off by at most 1/2 unit of 2^-16; it is multiplied by xo + 1/2 <= Wo - 1/2:
    less than (Wo - 1/2) * 2^-17.  mxy likewise with yo + 1/2 <= Ho - 1/2: less than (Ho - 1/2) * 2^-17.  Together (Wo + Ho - 1) * 2^-17;
  * tx is rounded once: 2^-17; the `>> 1` of the summed products drops at most 1/2 unit: 2^-17.  Together 2^-16;
  * the weight keeps 11 of the 16 fraction bits: x' lies below the fixed-point position by less than 2^-11.
So |x' - x| < e = 2^-11 + (Wo + Ho - 1) * 2^-17 + 2^-16, and the same e bounds |y' - y|.  f is continuous and piecewise linear along each
axis with a slope of at most 255 per pixel, hence |acc / 2^22 - f(y, x)| <= 255 (|x' - x| + |y' - y|) < 255 * 2 * e.  (float64 rounding of
the reference, ~1e-13, is far below the last digit of that and is not added.)

The colour matrix (`color_bound`): every Cm word is a real entry times 2^16 rounded, off by at most 2^-17 of a unit gain, times at most 255
grey levels, three of them per channel; Co is rounded once, 2^-17 grey level.  Before the final clamp (which never increases a distance)
|u / 2^38 - (M x + o)| <= (3 * 255 + 1) * 2^-17.
"""
import numpy as np

import helpers_augment as HA

NPARAM = 20
PAD_LABEL = HA.PAD_LABEL
MEAN_BGR = HA.MEAN_BGR
IDENTITY_COLOR = [65536, 0, 0, 0, 65536, 0, 0, 0, 65536, 0, 0, 0]
LUMA = np.array([0.299, 0.587, 0.114])


def bridge(rec9, out_hw, color=IDENTITY_COLOR):
    """the 9-word record of szn_augment_u8 (helpers_augment.record) -> the affine record with the same source positions"""
    h, w, _, _, step_y, step_x, oy, ox, flip = [int(v) for v in rec9]
    Wo = int(out_hw[1])
    return [h, w, -step_x if flip else step_x, 0, step_x * (ox + (Wo if flip else 0)), 0, step_y, step_y * oy] + [int(v) for v in color]


def affine_float(h, w, s, phi, oy=0.0, ox=0.0, flip=False, out_hw=None):
    """the host geometry in float64 (module docstring) -> (A (2,2), t (2,)): source continuous point = A (xo + 1/2, yo + 1/2) + t; row 0 is
    x, row 1 is y.  Quarter turns are exact (a cosine or sine below 1e-15 is 0)."""
    Hs, Ws = HA.record(h, w, s)[2:4]
    c, sn = np.cos(np.deg2rad(phi)), np.sin(np.deg2rad(phi))
    c, sn = (0.0 if abs(c) < 1e-15 else c), (0.0 if abs(sn) < 1e-15 else sn)
    Wb, Hb = abs(c) * Ws + abs(sn) * Hs, abs(sn) * Ws + abs(c) * Hs
    A = np.array([[w / Ws * c, w / Ws * sn], [-(h / Hs) * sn, h / Hs * c]])
    org = np.array([ox + (out_hw[1] if flip else 0) - Wb / 2.0, oy - Hb / 2.0])
    t = A @ org + np.array([w / 2.0, h / 2.0])
    if flip:
        A[:, 0] = -A[:, 0]
    return A, t


def box(h, w, s, phi):
    """(Hb, Wb) of the bounding box of the scaled, rotated image"""
    Hs, Ws = HA.record(h, w, s)[2:4]
    c, sn = abs(np.cos(np.deg2rad(phi))), abs(np.sin(np.deg2rad(phi)))
    return sn * Ws + c * Hs, c * Ws + sn * Hs


def affine_words(h, w, A, t, color=IDENTITY_COLOR):
    """float map -> the record, every coefficient rounded once"""
    q = np.rint(65536.0 * np.array([A[0, 0], A[0, 1], t[0], A[1, 0], A[1, 1], t[1]]))
    return [int(h), int(w)] + [int(v) for v in q] + [int(v) for v in color]


def positions(rec, out_hw):
    """the unclamped 16.16 source positions (sx, sy), int64 (Ho, Wo)"""
    Ho, Wo = out_hw
    X = (2 * np.arange(Wo, dtype=np.int64) + 1)[None, :]
    Y = (2 * np.arange(Ho, dtype=np.int64) + 1)[:, None]
    mxx, mxy, tx, myx, myy, ty = [np.int64(int(v)) for v in rec[2:8]]
    sx = ((mxx * X + mxy * Y) >> 1) + tx - 32768
    sy = ((myx * X + myy * Y) >> 1) + ty - 32768
    return sx, sy


def fixed_point(img, label, rec, out_hw):
    """one image: uint8 canvas (Hm,Wm,3), label (Hm,Wm), record -> (u int64 (Ho,Wo,3) RGB order = colour value * 2^38, label int64 (Ho,Wo),
    pad bool (Ho,Wo), acc int64 (Ho,Wo,3) = interpolated source bytes * 2^22); u is 0 where pad.  h, w are clamped to the canvas and the
    matrix words to +-2^20, as the contract has the device do."""
    Hm, Wm = np.asarray(img).shape[:2]
    h, w = min(max(int(rec[0]), 1), Hm), min(max(int(rec[1]), 1), Wm)
    sx, sy = positions(rec, out_hw)
    lx, ly = (sx + 32768) >> 16, (sy + 32768) >> 16
    pad = (lx < 0) | (lx >= w) | (ly < 0) | (ly >= h)
    cx, cy = np.clip(sx, 0, np.int64(w - 1) << 16), np.clip(sy, 0, np.int64(h - 1) << 16)
    x0, y0 = cx >> 16, cy >> 16
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    wx, wy = ((cx & 0xffff) >> 5)[..., None], ((cy & 0xffff) >> 5)[..., None]
    p = np.asarray(img).astype(np.int64)
    acc = (2048 - wy) * ((2048 - wx) * p[y0, x0] + wx * p[y0, x1]) + wy * ((2048 - wx) * p[y1, x0] + wx * p[y1, x1])
    assert acc.max() <= 255 << 22 and acc.min() >= 0
    cm = np.clip(np.array([int(v) for v in rec[8:17]], dtype=np.int64), -(1 << 20), 1 << 20).reshape(3, 3)
    co = np.array([int(v) for v in rec[17:20]], dtype=np.int64) << 22
    u = np.stack([cm[c, 0] * acc[..., 0] + cm[c, 1] * acc[..., 1] + cm[c, 2] * acc[..., 2] + co[c] for c in range(3)], axis=-1)
    u = np.clip(u, 0, np.int64(255) << 38)
    u[pad] = 0
    lab = np.asarray(label).astype(np.int64)[np.clip(ly, 0, h - 1), np.clip(lx, 0, w - 1)]
    lab[pad] = PAD_LABEL
    return u, lab, pad, acc


def augment(img, label, params, out_hw, mean_bgr=MEAN_BGR):
    """the batch: uint8 (B,Hm,Wm,3), labels (B,Hm,Wm), records (B,NPARAM) -> (float32 (B,3,Ho,Wo) BGR minus mean, int64 (B,Ho,Wo));
    padding is exactly 0.0 / PAD_LABEL"""
    B = len(img)
    Ho, Wo = out_hw
    data = np.zeros((B, 3, Ho, Wo), dtype=np.float32)
    target = np.empty((B, Ho, Wo), dtype=np.int64)
    mean = np.asarray(mean_bgr, dtype=np.float64)
    for b in range(B):
        u, lab, pad, _ = fixed_point(img[b], label[b], params[b], out_hw)
        bgr = (u[:, :, ::-1].astype(np.float64) / 274877906944.0 - mean).astype(np.float32)
        bgr[pad] = 0.0
        data[b] = bgr.transpose(2, 0, 1)
        target[b] = lab
    return data, target


def exact_bilinear(img, h, w, A, t, out_hw):
    """float64 bilinear interpolation of the top-left h x w of the canvas at the UNROUNDED affine positions -> (f (Ho,Wo,3) RGB,
    inside bool (Ho,Wo)): inside is the contract's padding rule on the real position, floor(x + 1/2) in [0, w) and the same in y"""
    Ho, Wo = out_hw
    xc = (np.arange(Wo, dtype=np.float64) + 0.5)[None, :]
    yc = (np.arange(Ho, dtype=np.float64) + 0.5)[:, None]
    x = A[0, 0] * xc + A[0, 1] * yc + t[0] - 0.5
    y = A[1, 0] * xc + A[1, 1] * yc + t[1] - 0.5
    nx, ny = np.floor(x + 0.5), np.floor(y + 0.5)
    inside = (nx >= 0) & (nx < w) & (ny >= 0) & (ny < h)
    x, y = np.clip(x, 0, w - 1), np.clip(y, 0, h - 1)
    x0, y0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    fx, fy = (x - x0)[..., None], (y - y0)[..., None]
    p = np.asarray(img).astype(np.float64)
    f = (1 - fy) * ((1 - fx) * p[y0, x0] + fx * p[y0, x1]) + fy * ((1 - fx) * p[y1, x0] + fx * p[y1, x1])
    return f, inside


def interp_bound(Ho, Wo):
    """upper bound of |acc / 2^22 - exact bilinear interpolation at the unrounded affine position| in grey levels (module docstring)"""
    e = 2.0 ** -11 + (Wo + Ho - 1) * 2.0 ** -17 + 2.0 ** -16
    return 255.0 * 2.0 * e


def photometric_chain(x, b=0.0, alpha=1.0, sigma=1.0, theta=0.0, mean_bgr=MEAN_BGR):
    """the four stages one after the other in float64 on RGB grey levels x (..., 3), one clamp to [0, 255] at the end: brightness x + 255 b;
    contrast about the mean colour m + alpha (x - m); saturation g + sigma (x - g) with the luma g; hue, the rotation by theta degrees
    about the grey axis (Rodrigues: x cos + (k x x) sin + k (k . x)(1 - cos), k = (1,1,1) / sqrt 3)"""
    x = np.asarray(x, dtype=np.float64)
    m = np.asarray(mean_bgr, dtype=np.float64)[::-1]
    x = x + 255.0 * b
    x = m + alpha * (x - m)
    g = (x * LUMA).sum(axis=-1, keepdims=True)
    x = g + sigma * (x - g)
    t = np.deg2rad(theta)
    k = np.ones(3) / np.sqrt(3.0)
    x = x * np.cos(t) + np.cross(np.broadcast_to(k, x.shape), x) * np.sin(t) + k * (x @ k)[..., None] * (1.0 - np.cos(t))
    return np.clip(x, 0.0, 255.0)


def color_bound():
    """upper bound of |u / 2^38 - the real-valued colour map| in grey levels (module docstring)"""
    return (3 * 255 + 1) * 2.0 ** -17
