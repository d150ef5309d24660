"""The reference of tests/helpers_accum.py tied down on the CPU: A backward() calls without zero_grad() on a two-layer conv net leave
helpers_accum.accumulate's left-to-right float32 sum in `.grad`, bit for bit; and dividing that sum by A before optim.step() is the
float64 Adam / SGD step of tests/helpers_state.py fed the mean, within those references' own bounds (the moment bounds, and the master
gate formed from the float32 restatement on the same inputs)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers_accum as A  # noqa: E402
import helpers_state as H  # noqa: E402

STEPS = 3


def net(seed=5):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, padding=1), torch.nn.ReLU(), torch.nn.Conv2d(8, 4, 3, padding=1))


def batches(steps=STEPS):
    g = torch.Generator().manual_seed(11)
    return [(torch.randn(2, 3, 12, 10, generator=g) * 10.0 ** (k - 1), torch.randn(2, 4, 12, 10, generator=g)) for k in range(steps)]


def loss(m, x, y):
    return ((m(x) - y) ** 2).mean()


def micro_grads(m, data):
    """every micro-batch's own gradient (zero_grad in between), per parameter: [steps][params] numpy arrays"""
    out = []
    for x, y in data:
        m.zero_grad(set_to_none=True)
        loss(m, x, y).backward()
        out.append([p.grad.numpy().copy() for p in m.parameters()])
    m.zero_grad(set_to_none=True)
    return out


def accumulated(m, data):
    m.zero_grad(set_to_none=True)
    for x, y in data:
        loss(m, x, y).backward()
    return [p.grad.numpy().copy() for p in m.parameters()]


def test_helper_adds_left_to_right_in_float32():
    a, b, c = np.array([2.0 ** 24], np.float32), np.array([1.0], np.float32), np.array([1.0], np.float32)
    assert A.accumulate([a, b, c])[0] == 2.0 ** 24                 # (2^24 + 1) + 1: both additions round back
    assert A.accumulate([b, c, a])[0] == 2.0 ** 24 + 2             # (1 + 1) + 2^24 is exact
    assert A.accumulate([a, b, c, c], average=True)[0] == 2.0 ** 22
    x, y = A.special_pair(64, 3)
    s = A.accumulate([x, y])
    i = np.arange(6) * 8 + 1
    assert np.isnan(s[i[0]]) and s[i[1]] == np.inf and np.isnan(s[i[2]])
    assert np.signbit(s[i[3]]) and s[i[4]] == 0 and not np.signbit(s[i[4]]) and s[i[5]] == 0 and not np.signbit(s[i[5]])
    assert A.same_floats(s, s.copy()) and not A.same_floats(s, np.where(np.isnan(s), np.float32(1), s))


def test_backward_without_zero_grad_is_the_helper_sum_bit_for_bit():
    m, data = net(), batches()
    gs = micro_grads(m, data)
    got = accumulated(m, data)
    rounded = 0
    for k, g in enumerate(got):
        want = A.accumulate([gs[t][k] for t in range(STEPS)])
        assert np.array_equal(g.view(np.int32), want.view(np.int32)), k
        exact = sum(gs[t][k].astype(np.float64) for t in range(STEPS))
        rounded += int((want.astype(np.float64) != exact).sum())
    assert rounded > 0                                              # the additions really round on these inputs


@pytest.mark.parametrize("opt", ["adam", "sgd"])
def test_mean_then_step_is_the_float64_reference_fed_the_mean(opt):
    m, data = net(), batches()
    gs = micro_grads(m, data)
    params = list(m.parameters())
    p0 = [p.detach().numpy().copy() for p in params]
    hp = H.ADAM_HP
    wd = H.ADAM_WDS[1] if opt == "adam" else H.SGD_WDS[1]
    if opt == "adam":
        o = torch.optim.Adam(params, lr=H.f32v(hp["lr"]), betas=(H.f32v(hp["b1"]), H.f32v(hp["b2"])), eps=H.f32v(hp["eps"]),
                             weight_decay=H.f32v(wd), foreach=False)
    else:
        o = torch.optim.SGD(params, lr=H.f32v(H.SGD_LR), momentum=H.f32v(H.SGD_MOMENTUM), weight_decay=H.f32v(wd), foreach=False)
    m.zero_grad(set_to_none=True)
    for x, y in data:
        loss(m, x, y).backward()
    for p in params:
        p.grad.div_(STEPS)
    means = [p.grad.numpy().copy() for p in params]
    o.step()
    for k, p in enumerate(params):
        mean = A.accumulate([gs[t][k] for t in range(STEPS)], average=True)
        assert np.array_equal(means[k].view(np.int32), mean.view(np.int32)), k
        zero = np.zeros_like(p0[k])
        got = p.detach().numpy()
        if opt == "adam":
            a = (p0[k], mean, zero, zero, hp["lr"], hp["b1"], hp["b2"], hp["eps"], wd, 1)
            p64, m64, v64 = H.adam_ref(*a)
            p32 = H.adam_f32(*a)[0]
            bm, bv = H.adam_moment_bounds(p0[k], mean, zero, zero, hp["b1"], hp["b2"], wd)
            st = o.state[p]
            assert np.all(np.abs(st["exp_avg"].numpy() - m64) <= bm) and np.all(np.abs(st["exp_avg_sq"].numpy() - v64) <= bv)
        else:
            a = (p0[k], mean, zero, H.SGD_LR, H.SGD_MOMENTUM, wd, True)
            p64, b64 = H.sgd_ref(*a)
            p32 = H.sgd_f32(*a)[0]
            assert np.all(np.abs(o.state[p]["momentum_buffer"].numpy() - b64) <= H.sgd_buf_bound(p0[k], mean, zero, H.SGD_MOMENTUM, wd, True))
        gate = H.master_gate(H.master_units(p32, p64, p0[k]))
        units = H.master_units(got, p64, p0[k])
        print("%s param %d: master error %.2f units, gate %.2f" % (opt, k, float(units.max()), gate))
        assert np.all(units <= gate)
        assert not np.array_equal(got, p0[k])
