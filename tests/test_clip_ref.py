"""CPU: the float64 restatement of gradient-norm clipping (tests/helpers_clip.py) against torch.nn.utils.clip_grad_norm_ on CPU tensors:
the norm, the coefficient min(1, MAX / (norm + 1e-6)) and the scaled gradients, at MAX below the norm, above it and MAX = inf."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers_clip as R  # noqa: E402

SHAPES = [(64, 3, 3, 3), (64,), (7, 5), (1,)]
SEG_END = np.cumsum([int(np.prod(s)) for s in SHAPES])


def grads(seed=3):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(s) * 10.0 ** rng.uniform(-3, 1) for s in SHAPES]


@pytest.mark.parametrize("which", ["below", "above", "inf"])
def test_coefficient_and_scaled_gradients_equal_torch(which):
    gs = grads()
    flat = np.concatenate([g.reshape(-1) for g in gs])
    stats, _ = R.stats_ref(flat, SEG_END)
    true_norm = math.sqrt(math.fsum(flat * flat))
    max_norm = {"below": 0.5 * true_norm, "above": 2.0 * true_norm, "inf": float("inf")}[which]
    max_norm = float(np.float32(max_norm))                       # the value a `float` argument carries
    coef, norm, finite = R.clip_ref(stats[:, 1], max_norm)
    assert finite and abs(norm - true_norm) <= 4 * R.U53 * true_norm
    params = [torch.nn.Parameter(torch.zeros(s, dtype=torch.float64)) for s in SHAPES]
    for p, g in zip(params, gs):
        p.grad = torch.from_numpy(g.copy())
    tnorm = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
    assert abs(tnorm - norm) <= 1e-14 * norm
    want = min(1.0, max_norm / (tnorm + 1e-6))
    assert abs(coef - want) <= 1e-14
    assert (coef < 1.0) == (which == "below") and (which == "below" or coef == 1.0)
    for p, g in zip(params, gs):
        assert np.allclose(p.grad.numpy(), g * coef, rtol=1e-13, atol=0.0)


def test_statistics_are_per_segment_and_handle_empty_segments():
    flat = np.arange(1.0, 11.0)
    stats, mag = R.stats_ref(flat, [1, 3, 3, 10])
    assert stats.tolist() == [[1.0, 1.0], [5.0, 13.0], [0.0, 0.0], [49.0, 371.0]] and mag.tolist() == [1.0, 5.0, 0.0, 49.0]
    bs, bq = R.stats_bounds([1, 3, 3, 10], stats, mag)
    assert bs[2] == 0.0 and bq[3] == (7 + 64) * R.U53 * 371.0


def test_a_non_finite_total_keeps_coef_at_one():
    for bad in (float("inf"), float("nan")):
        coef, norm, finite = R.clip_ref([1.0, bad], 0.5, 0.125, 1024.0)
        assert coef == 1.0 and not finite and not math.isfinite(norm)


def test_loss_scale_and_grad_scale_enter_the_norm():
    coef, norm, _ = R.clip_ref([9.0, 16.0], 0.0001, 0.125, 1024.0)
    assert norm == 5.0 * 0.125 / 1024.0 and coef == float(np.float32(0.0001)) / (norm + 1e-6) < 1.0
    assert R.clip_ref([9.0, 16.0], 0.001, 0.125, 1024.0)[0] == 1.0


def test_clipped_update_is_the_plain_update_with_the_scaled_gradient():
    rng = np.random.default_rng(5)
    p, g, m, v = (rng.standard_normal(9).astype(np.float32) for _ in range(4))
    v = np.abs(v)
    coef = float(np.float32(0.37))
    a = R.adam_clipped_ref(p, g, m, v, coef, 1e-3, 0.9, 0.999, 1e-8, 0.0, 3, grad_scale=0.5)
    b = R.adam_ref(p, g.astype(np.float64) * (0.5 * coef), m, v, 1e-3, 0.9, 0.999, 1e-8, 0.0, 3)
    for x, y in zip(a, b):
        assert np.allclose(x, y, rtol=1e-6, atol=0)               # (the product 0.5 * coef is rounded to float32 in the restatement)
    s = R.sgd_clipped_ref(p, g, m, coef, 1e-2, 0.99, 0.0, False, grad_scale=0.5)
    t = R.sgd_ref(p, g.astype(np.float64) * (0.5 * coef), m, 1e-2, 0.99, 0.0, False)
    for x, y in zip(s, t):
        assert np.allclose(x, y, rtol=1e-6, atol=1e-12)
