"""The float64 references of tests/helpers_state.py, tied down on the CPU: adam_ref / sgd_ref against torch.optim in float64, the
float32 restatements inside the gates that tests/test_gpu_state_kernels.py applies to the kernels (on that file's own inputs), the
Dropout2d generator's statistics and the loss-scale state machine on a hand-written trace."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers_state as H  # noqa: E402


def _torch_adam(p0, grads, m0, v0, betas, wd):
    p = torch.nn.Parameter(torch.from_numpy(p0.astype(np.float64)))
    opt = torch.optim.Adam([p], lr=H.f32v(H.ADAM_HP["lr"]), betas=betas, eps=H.f32v(H.ADAM_HP["eps"]), weight_decay=H.f32v(wd),
                           foreach=False)
    opt.state[p] = dict(step=torch.tensor(0.0), exp_avg=torch.from_numpy(m0.astype(np.float64)),
                        exp_avg_sq=torch.from_numpy(v0.astype(np.float64)))
    out = []
    for g in grads:
        p.grad = torch.from_numpy(g.astype(np.float64))
        opt.step()
        st = opt.state[p]
        out.append((p.detach().numpy().copy(), st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy()))
    return out


def _state_inputs(n=4096, seed=3, steps=5):
    """moments of a previous step whose gradient had the sign of this one's (no cancellation in m: the RELATIVE difference of an
    update is then a meaningful number)"""
    rng = np.random.default_rng(seed)
    p0 = (rng.standard_normal(n) * 0.02).astype(np.float32)
    sign = rng.choice([-1.0, 1.0], n)
    grads = [(sign * 10.0 ** rng.uniform(-4, 0, n)).astype(np.float32) for _ in range(steps + 1)]
    m0 = (0.1 * grads[0]).astype(np.float32)
    v0 = (0.001 * grads[0].astype(np.float64) ** 2).astype(np.float32)
    return p0, grads[1:], m0, v0


@pytest.mark.parametrize("wd", H.ADAM_WDS)
def test_adam_ref_is_torch_adam_in_float64_with_float32_valued_betas(wd):
    p0, grads, m0, v0 = _state_inputs()
    hp = H.ADAM_HP
    want = _torch_adam(p0, grads, m0, v0, (H.f32v(hp["b1"]), H.f32v(hp["b2"])), wd)
    p, m, v = p0.astype(np.float64), m0.astype(np.float64), v0.astype(np.float64)
    for t, g in enumerate(grads, 1):
        p, m, v = H.adam_ref(p, g, m, v, hp["lr"], hp["b1"], hp["b2"], hp["eps"], wd, t)
        tp, tm, tv = want[t - 1]
        np.testing.assert_allclose(p, tp, rtol=1e-12, atol=0)
        np.testing.assert_allclose(m, tm, rtol=1e-12, atol=0)
        np.testing.assert_allclose(v, tv, rtol=1e-12, atol=0)


def test_distance_to_torch_adam_with_literal_betas():
    """torch.optim.Adam(betas=(0.9, 0.999)) uses the Python doubles; the C interface carries float32(0.999), and
    (1 - f32(0.999)) / (1 - 0.999) - 1 = -1.3e-5.  At step 1 the update is lr (b1/(1-b1) m0 + g) / (sqrt(b2/(1-b2) v0 + g^2) + eps): only
    the ratio b2/(1-b2) under the square root moves by 1.3e-5 (half of it survives the root), b1/(1-b1) by 2.7e-7: below 1.3e-5."""
    p0, grads, m0, v0 = _state_inputs()
    hp = H.ADAM_HP
    a = _torch_adam(p0, grads, m0, v0, (H.f32v(hp["b1"]), H.f32v(hp["b2"])), 0.0)
    b = _torch_adam(p0, grads, m0, v0, (0.9, 0.999), 0.0)
    prev_a = prev_b = p0.astype(np.float64)
    rel = []
    for (pa, _, _), (pb, _, _) in zip(a, b):
        ua, ub = pa - prev_a, pb - prev_b
        rel.append(float(np.max(np.abs(ub - ua) / np.abs(ua))))
        prev_a, prev_b = pa, pb
    print("relative difference of the Adam update, float32-valued vs literal betas, steps 1..5: " + " ".join("%.3g" % r for r in rel))
    assert 0.0 < rel[0] < 1.3e-5


@pytest.mark.parametrize("wd", H.SGD_WDS)
def test_sgd_ref_is_torch_sgd_in_float64(wd):
    p0, grads, _, _ = _state_inputs()
    p = torch.nn.Parameter(torch.from_numpy(p0.astype(np.float64)))
    opt = torch.optim.SGD([p], lr=H.f32v(H.SGD_LR), momentum=H.f32v(H.SGD_MOMENTUM), weight_decay=H.f32v(wd), foreach=False)
    q, buf = p0.astype(np.float64), np.full(p0.shape, np.nan)           # first_step must not read the old buffer
    for t, g in enumerate(grads):
        p.grad = torch.from_numpy(g.astype(np.float64))
        opt.step()
        q, buf = H.sgd_ref(q, g, buf, H.SGD_LR, H.SGD_MOMENTUM, wd, t == 0)
        np.testing.assert_allclose(q, p.detach().numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(buf, opt.state[p]["momentum_buffer"].numpy(), rtol=1e-12, atol=0)


@pytest.mark.parametrize("n", H.SIZES)
def test_float32_adam_restatement_stays_inside_the_gates(n):
    """the reference alone stays inside the gate: on the GPU test's own inputs the op-by-op float32 chain fits the derived moment
    bounds, and its master error in units of ulp(p) + 2^-23 |dp| (the number the GPU gate doubles) is small and printed"""
    x = H.opt_inputs(n, seed=n)
    hp = H.ADAM_HP
    worst = {}
    for step, wd, gs in itertools.product(H.ADAM_STEPS, H.ADAM_WDS, H.GRAD_SCALES):
        a = (x["p"], x["g"], x["m"], x["v"], hp["lr"], hp["b1"], hp["b2"], hp["eps"], wd, step, gs)
        p64, m64, v64 = H.adam_ref(*a)
        p32, m32, v32 = H.adam_f32(*a)
        bm, bv = H.adam_moment_bounds(x["p"], x["g"], x["m"], x["v"], hp["b1"], hp["b2"], wd, gs)
        assert np.all(np.abs(m32 - m64) <= bm), (step, wd, gs)
        assert np.all(np.abs(v32 - v64) <= bv), (step, wd, gs)
        units = H.master_units(p32, p64, x["p"])
        worst[step] = max(worst.get(step, 0.0), float(units.max()))
        if wd == 0.0:
            assert np.array_equal(p32[x["zero"]], x["p"][x["zero"]])
    print("n=%d adam_f32 master error in units, worst per step: %s" % (n, " ".join("%d:%.2f" % kv for kv in sorted(worst.items()))))
    assert np.isfinite(max(worst.values()))    # (no gate here: the GPU gate is 2 x this figure + 1, formed on the same inputs)


@pytest.mark.parametrize("n", H.SIZES)
def test_float32_sgd_restatement_stays_inside_the_gates(n):
    x = H.opt_inputs(n, seed=n)
    worst = 0.0
    for first, wd, lr in itertools.product((1, 0), H.SGD_WDS, (H.SGD_LR, 2 * H.SGD_LR)):
        buf0 = np.full(n, np.nan, np.float32) if first else x["buf"]
        a = (x["p"], x["g"], buf0, lr, H.SGD_MOMENTUM, wd, first)
        p64, b64 = H.sgd_ref(*a)
        p32, b32 = H.sgd_f32(*a)
        assert np.all(np.isfinite(p32)) and np.all(np.isfinite(b32))
        assert np.all(np.abs(b32 - b64) <= H.sgd_buf_bound(x["p"], x["g"], buf0, H.SGD_MOMENTUM, wd, first))
        if first and wd == 0.0:
            assert np.array_equal(b32, x["g"])
        worst = max(worst, float(H.master_units(p32, p64, x["p"]).max()))
    print("n=%d sgd_f32 master error in units, worst: %.2f" % (n, worst))
    assert np.isfinite(worst)


def test_dropout_ref_keep_rate_and_independence():
    """p = 0.5, n = 2^20: keep rate within 5 sigma of the binomial (sigma = sqrt(.25 / n) = 4.9e-4) for the seeds of ranks 0 and 1 and
    the offsets of the first four calls (k << 24); any two of the eight masks agree on 0.5 +- 5 sigma of the positions"""
    n = 2 ** 20
    sigma = np.sqrt(0.25 / n)
    masks = []
    for seed in (1337, 1337 + 7919):
        for k in range(4):
            mk = H.dropout_ref(n, 0.5, seed, k << 24)
            assert set(np.unique(mk)) == {0.0, 2.0}
            rate = float((mk != 0).mean())
            print("seed %d offset %d<<24: keep rate %.5f" % (seed, k, rate))
            assert abs(rate - 0.5) <= 5 * sigma
            masks.append(mk != 0)
    for a, b in itertools.combinations(range(8), 2):
        agree = float((masks[a] == masks[b]).mean())
        assert abs(agree - 0.5) <= 5 * sigma, (a, b, agree)
    assert np.all(H.dropout_ref(1000, 0.0, 5, 0) == 1.0)
    # the offset contract: the stream of (seed, offset + k) is the stream of (seed, offset) moved by k
    assert np.array_equal(H.dropout_ref(1000, 0.25, 9, 77 + 13), H.dropout_ref(1013, 0.25, 9, 77)[13:])


def test_loss_scale_model_follows_its_contract_on_a_trace():
    def run(state, flags, *cfg):
        out = []
        for f in flags:
            state = np.array([state[0], f, state[2], state[3]], np.float32)
            state = H.loss_scale_model(state, *cfg)
            out.append(tuple(float(x) for x in state))
        return out
    # interval 3: two clean steps, an overflow (count restarts, step not counted), three clean steps -> growth
    assert run([8.0, 0, 10, 0], [0, 0, 1, 0, 0, 0], 2.0, 0.5, 3, 1.0, 64.0) == [
        (8, 0, 11, 1), (8, 0, 12, 2), (4, 0, 12, 0), (4, 0, 13, 1), (4, 0, 14, 2), (8, 0, 15, 0)]
    # overflows at the floor: S holds
    assert run([2.0, 0, 0, 5], [1, 1, 1], 2.0, 0.5, 3, 1.0, 64.0) == [(1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 0, 0)]
    # growth at the ceiling, interval 1: every clean step grows, S stops at hi
    assert run([16.0, 0, 0, 0], [0, 0, 0, 0], 2.0, 0.5, 1, 1.0, 48.0) == [(32, 0, 1, 0), (48, 0, 2, 0), (48, 0, 3, 0), (48, 0, 4, 0)]
    # a scale above the ceiling is not lowered by growth, only by an overflow
    assert run([128.0, 0, 0, 0], [0, 1], 2.0, 0.5, 1, 1.0, 48.0) == [(128, 0, 1, 0), (64, 0, 1, 0)]
