"""float64 restatement of the gradient statistics, the clipping coefficient and the clipped update (include/szn.h: szn_grad_stats,
szn_clip_coef, szn_*_step_clipped), in plain numpy.  tests/test_clip_ref.py ties it to torch.nn.utils.clip_grad_norm_;
tests/test_gpu_clip.py and tests/test_gpu_clip_model.py hold the kernels and the engine against it.  Nothing here touches a GPU."""
import math

import numpy as np

from helpers_state import F32, F64, adam_ref, f32v, sgd_ref

U53 = 2.0 ** -53                   # unit round-off of float64


def segments(seg_end):
    """[(lo, hi)] of a segment table: segment s = [seg_end[s-1], seg_end[s])"""
    lo = 0
    for hi in seg_end:
        yield lo, int(hi)
        lo = int(hi)


def stats_ref(g, seg_end):
    """-> (stats [n_seg][2] = {sum g, sum g*g}, sum |g| per segment), each by math.fsum over the exactly widened elements: the
    correctly rounded value of the exact sum (g*g is exact in float64 for fp32 / bf16 / f16 inputs)"""
    g = np.asarray(g, F64)
    out, mag = [], []
    for lo, hi in segments(seg_end):
        s = g[lo:hi]
        out.append((math.fsum(s), math.fsum(s * s)))
        mag.append(math.fsum(np.abs(s)))
    return np.array(out, F64).reshape(-1, 2), np.array(mag, F64)


def stats_bounds(seg_end, stats, mag):
    """per segment of length m: the additions in double are the only roundings, at most m + 64 of them in a row on any path to the result
    -> |sumsq - exact| <= (m + 64) 2^-53 exact, |sum - exact| <= (m + 64) 2^-53 sum |g|"""
    m = np.array([hi - lo for lo, hi in segments(seg_end)], F64)
    return (m + 64) * U53 * mag, (m + 64) * U53 * stats[:, 1]


def clip_ref(sumsq, max_norm, grad_scale=1.0, loss_scale=1.0):
    """szn_clip_coef in float64 from the per-segment sums of squares -> (coef, norm, finite).  The float arguments carry their float32
    values.  Not finite: coef 1, the norm as it comes out."""
    total = 0.0
    for q in sumsq:
        total += float(q)
    with np.errstate(invalid="ignore"):
        norm = float(np.sqrt(F64(total))) * f32v(grad_scale) / f32v(loss_scale)
    if not math.isfinite(total):
        return 1.0, norm, False
    mx = f32v(max_norm)
    return (mx / (norm + 1e-6) if norm + 1e-6 > mx else 1.0), norm, True


def adam_clipped_ref(p, g, m, v, coef, lr, b1, b2, eps, wd, step, grad_scale=1.0, loss_scale=1.0):
    """the clipped Adam step: adam_ref with the gradient scale times the coefficient (coef as the float32 the device holds)"""
    return adam_ref(p, g, m, v, lr, b1, b2, eps, wd, step, f32v(grad_scale) * f32v(coef), loss_scale)


def sgd_clipped_ref(p, g, buf, coef, lr, momentum, wd, first_step, grad_scale=1.0, loss_scale=1.0):
    return sgd_ref(p, g, buf, lr, momentum, wd, first_step, f32v(grad_scale) * f32v(coef), loss_scale)


def f32_neighbours(x):
    """float32(x) and its two neighbours, as a set of floats"""
    c = F32(x)
    return {float(c), float(np.nextafter(c, F32(np.inf))), float(np.nextafter(c, F32(-np.inf)))}
