"""CPU: the float64 reference of the averaged-weights recurrence (tests/helpers_ema.py) pinned against the closed form for constant
parameters and against torch's own exponential moving average."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers_ema as R  # noqa: E402


def test_factor_warmup_and_every():
    assert R.ema_factor(0.999, 1, 0) == 0.1 and R.ema_factor(0.999, 1, 0, warmup=False) == float(np.float32(0.999))
    assert R.ema_factor(0.5, 1, 7) == 8.0 / 17.0 and R.ema_factor(0.5, 1, 20) == 0.5      # the ramp is below decay only at the start
    assert R.ema_factor(0.9, 4, 100) == (101.0 / 110.0 if 101.0 / 110.0 < float(np.float32(0.9)) else float(np.float32(0.9))) ** 4
    s = 10 ** 6
    assert R.ema_factor(0.999, 3, s) == float(np.float32(0.999)) ** 3        # far along the ramp is above every decay < 1
    assert R.ema_factor(1.0, 2, 0, warmup=False) == 1.0 and R.ema_factor(0.0, 5, 3) == 0.0


@pytest.mark.parametrize("every,warmup", [(1, True), (1, False), (3, True), (4, False)])
def test_closed_form_for_constant_parameters(every, warmup):
    """avg_t - p = (avg_0 - p) * prod D_i"""
    rng = np.random.default_rng(3)
    p, a0 = rng.normal(size=50), rng.normal(size=50)
    T = 24
    run = R.ema_run(a0, [p] * T, 0.97, every, warmup)
    prod, s = 1.0, 0
    for t in range(1, T + 1):
        if t % every == 0:
            prod *= R.ema_factor(0.97, every, s, warmup)
        s += 1
        np.testing.assert_allclose(run[t - 1][0] - p, (a0 - p) * prod, rtol=1e-12, atol=1e-15)
    assert run[-1][3] == T // every
    assert all((D is None) == bool(t % every) for t, (_, _, D, _) in enumerate(run, 1))


def test_skipped_steps_neither_update_nor_count():
    rng = np.random.default_rng(4)
    a0 = rng.normal(size=8)
    ps = [rng.normal(size=8) for _ in range(6)]
    applied = [False, False, True, False, True, True]
    run = R.ema_run(a0, ps, 0.9, 1, True, applied)
    assert np.array_equal(run[0][0], a0) and np.array_equal(run[1][0], a0) and run[0][2] is None
    assert run[2][2] == R.ema_factor(0.9, 1, 0) and np.array_equal(run[3][0], run[2][0])       # the first applied step: s = 0
    assert run[4][2] == R.ema_factor(0.9, 1, 1) and run[5][2] == R.ema_factor(0.9, 1, 2)
    # every = 2: the boundaries are attempted steps 2, 4, 6; step 2 and 4 were skipped -> one update, with s = 2
    run2 = R.ema_run(a0, ps, 0.9, 2, True, applied)
    assert [r[2] for r in run2] == [None] * 5 + [R.ema_factor(0.9, 2, 2)] and run2[-1][3] == 3
    np.testing.assert_array_equal(run2[-1][0], R.ema_update(a0, ps[5], R.ema_factor(0.9, 2, 2)))


def test_against_torch_averaged_model():
    """warmup=False against torch.optim.swa_utils.AveragedModel with an EMA avg_fn (its first update copies the parameters: avg_0)"""
    decay = 0.75                                                             # exact in float32: both sides use the same number
    torch.manual_seed(0)
    net = torch.nn.Linear(5, 3).double()
    flat = lambda m: torch.cat([q.detach().reshape(-1) for q in m.parameters()]).numpy().copy()
    swa = getattr(torch.optim, "swa_utils", None)
    if swa is not None and hasattr(swa, "AveragedModel"):
        avg = swa.AveragedModel(net, avg_fn=lambda a, q, n: decay * a + (1.0 - decay) * q)
        avg.update_parameters(net)
        read = lambda: flat(avg.module)
        update = lambda: avg.update_parameters(net)
    else:                                                                    # the three-line restatement
        state = [q.detach().clone() for q in net.parameters()]
        read = lambda: torch.cat([a.reshape(-1) for a in state]).numpy().copy()
        update = lambda: [a.mul_(decay).add_(q.detach(), alpha=1.0 - decay) for a, q in zip(state, net.parameters())]
    a0, ps, want = read(), [], []
    for _ in range(12):
        with torch.no_grad():
            for q in net.parameters():
                q.add_(torch.randn_like(q) * 0.1)
        update()
        ps.append(flat(net))
        want.append(read())
    run = R.ema_run(a0, ps, decay, 1, warmup=False)
    for (got, _, D, _), w in zip(run, want):
        assert D == decay
        np.testing.assert_allclose(got, w, rtol=1e-13, atol=1e-15)


def test_bound_accumulates_with_the_factor():
    a0, p = np.array([2.0, -1.0]), np.array([1.0, 4.0])
    run = R.ema_run(a0, [p, p], 0.5, 1, warmup=False)
    b1 = 4 * R.EPS * np.array([2.0, 4.0])
    np.testing.assert_allclose(run[0][1], b1)
    np.testing.assert_allclose(run[1][1], 0.5 * b1 + 4 * R.EPS * np.maximum(np.abs(run[0][0]), np.abs(p)))
