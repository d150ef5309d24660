"""GPU: szn_ema_step and szn_swap_f32 through the C interface -- the averaged-weights update against the float64 recurrence
(tests/helpers_ema.py) with the derived per-element bound, its exact corners, the device-side skip contract of the dynamic loss scale,
and the bit-exact exchange.  Sizes cross the kernels' paths: a lone scalar, less than one vector, one vector, around one 256-thread
block, several blocks with a tail, and 2^20 + 5 elements (513 blocks of vector pairs, lanes with an odd last vector); slices at [1:] move
a pointer off its 16-byte boundary (both: scalar head + vector body; one: the all-scalar path).  All of those finish in one round of
the kernels' loops; test_grid_stride_rounds holds the two sizes past the largest grid, where lanes take a second round."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers_ema as R  # noqa: E402
from zeroshotsemanticsegmentation_amd import _lib as L  # noqa: E402

SIZES = [1, 3, 4, 255, 256, 257, 1023, 4099, 2 ** 20 + 5]
OFFSETS = [(0, 0), (1, 1), (1, 0), (0, 1)]


def dev(a, off):
    """`a` on the GPU behind `off` spare elements: off = 1 puts it 4 bytes past a 16-byte boundary"""
    base = torch.empty(a.size + off, dtype=torch.from_numpy(a[:0]).dtype, device="cuda")
    assert base.data_ptr() % 16 == 0
    t = base[off:]
    t.copy_(torch.from_numpy(a))
    return t


def ema(avg, p, decay, every=1, step=0, state=None):
    L.call("szn_ema_step", avg.numel(), L.ptr(avg), L.ptr(p), decay, every, step, L.ptr(state), L.stream_ptr())


def bits(t):
    return t.view(torch.int32).cpu().numpy().copy()


@pytest.mark.parametrize("n", SIZES)
def test_update_against_float64_reference(n):
    rng = np.random.default_rng(n)
    a0, p0 = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    bound = R.ema_step_bound(a0, p0)
    worst = 0.0
    for oa, op in OFFSETS:
        p = dev(p0, op)
        for decay in (0.9, 0.999):
            for every in (1, 4):
                for step in (0, 1, 2, 50):
                    avg = dev(a0, oa)
                    ema(avg, p, decay, every, step)
                    assert L.last_kernel() == "ema_kernel"
                    want = R.ema_update(a0, p0, R.ema_factor(decay, every, step - 1, warmup=step > 0))
                    err = np.abs(avg.cpu().numpy().astype(np.float64) - want)
                    worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
                    assert (err <= bound).all(), (oa, op, decay, every, step, float((err / bound).max()))
        assert np.array_equal(p.cpu().numpy(), p0)                           # the parameters are only read
    print("n = %d: largest error %.3f of the bound 4 * 2^-24 * max(|avg|, |param|)" % (n, worst))


@pytest.mark.parametrize("n", [1, 257, 4099])
@pytest.mark.parametrize("off", OFFSETS)
def test_exact_corners(n, off):
    rng = np.random.default_rng(7 + n)
    a0, p0 = rng.standard_normal(n).astype(np.float32), (rng.standard_normal(n) * 1e3).astype(np.float32)
    p = dev(p0, off[1])
    avg = dev(a0, off[0])
    ema(avg, p, 1.0, 3, 0)                                                   # decay = 1: nothing moves
    assert np.array_equal(bits(avg), a0.view(np.int32))
    ema(avg, p, 0.0, 1, 0)                                                   # decay = 0: a copy of the parameters
    assert np.array_equal(bits(avg), p0.view(np.int32))
    for decay, every, step in ((0.9, 1, 0), (0.999, 4, 7)):                  # avg == param is a fixed point
        ema(avg, p, decay, every, step)
        assert np.array_equal(bits(avg), p0.view(np.int32))


@pytest.mark.parametrize("every", [1, 2])
def test_twenty_chained_updates_with_warmup(every):
    n = 4099
    rng = np.random.default_rng(11)
    a0 = rng.standard_normal(n).astype(np.float32)
    ps = [rng.standard_normal(n).astype(np.float32) for _ in range(20)]
    avg = dev(a0, 1)
    p = dev(ps[0], 1)
    run = R.ema_run(a0, ps, 0.99, every, warmup=True)
    worst = 0.0
    for t, (want, bound, D, _) in enumerate(run, 1):
        if t % every:
            continue
        p.copy_(torch.from_numpy(ps[t - 1]))
        ema(avg, p, 0.99, every, t)
        err = np.abs(avg.cpu().numpy().astype(np.float64) - want)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (t, float((err / bound).max()))
    print("20 chained steps, every %d: largest error %.3f of the accumulated bound" % (every, worst))


@pytest.mark.parametrize("n,off", [(3, (0, 0)), (4099, (1, 1)), (4099, (0, 1)), (2 ** 20 + 5, (0, 0))])
def test_device_side_skip(n, off):
    rng = np.random.default_rng(13)
    a0, p0 = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    p = dev(p0, off[1])
    s = 7
    # found_inf set: the optimizer entries skipped this step, the average stays bit for bit
    avg = dev(a0, off[0])
    ema(avg, p, 0.9, 1, 3, torch.tensor([1024.0, 1.0, float(s), 0.0], device="cuda"))
    assert L.last_kernel() == "ema_kernel" and np.array_equal(bits(avg), a0.view(np.int32))
    # flag clear: s comes from scale_state[2], whatever step the host passes
    for decay, every in ((0.9, 1), (0.999, 4)):
        state = torch.tensor([1024.0, 0.0, float(s), 5.0], device="cuda")
        avg = dev(a0, off[0])
        ema(avg, p, decay, every, 3, state)
        static = dev(a0, off[0])
        ema(static, p, decay, every, s + 1)
        assert np.array_equal(bits(avg), bits(static)) and not np.array_equal(bits(avg), a0.view(np.int32))
        assert state.cpu().tolist() == [1024.0, 0.0, float(s), 5.0]          # the state is only read
        # step = 0 switches the warm-up off on this path too
        avg = dev(a0, off[0])
        ema(avg, p, decay, every, 0, state)
        static = dev(a0, off[0])
        ema(static, p, decay, every, 0)
        assert np.array_equal(bits(avg), bits(static))


GRID = (1 << 17) * 256          # lanes of the largest grid (EMA_MAX_BLOCKS blocks of 256): beyond it the kernels take further rounds


@pytest.mark.parametrize("n,off", [(12 * GRID + 2 ** 22 + 5, (0, 0)),        # vectors: a second round of pairs, then odd last vectors
                                   (GRID + 2 ** 20 + 5, (0, 1))],            # all-scalar: a second round of the scalar loop
                         ids=["vector-rounds", "scalar-rounds"])
def test_grid_stride_rounds(n, off):
    """the sizes at which a lane takes more than one round (the 135 M-element weight buffer is one round); reference and comparison in
    float64 on the device"""
    g = torch.Generator(device="cuda").manual_seed(n % 1000)
    base_a, base_p = (torch.randn(n + 1, device="cuda", generator=g) for _ in range(2))
    avg, p = base_a[off[0]:off[0] + n], base_p[off[1]:off[1] + n]
    a0, p0 = avg.clone(), p.clone()
    D = R.ema_factor(0.9, 1, 4)
    want, bound = R.ema_update(a0, p0, D), R.ema_step_bound(a0, p0)
    ema(avg, p, 0.9, 1, 5)
    err = (avg.double() - want).abs()
    assert bool((err <= bound).all()) and torch.equal(p, p0)
    print("n = %d: largest error %.3f of the bound" % (n, float((err / bound.clamp_min(1e-300)).max())))
    del want, bound, err
    avg.copy_(a0)
    avg[::7919] = float("nan")
    a0 = avg.clone()
    L.call("szn_swap_f32", n, L.ptr(avg), L.ptr(p), L.stream_ptr())
    assert torch.equal(avg.view(torch.int32), p0.view(torch.int32)) and torch.equal(p.view(torch.int32), a0.view(torch.int32))


def test_ema_bad_arguments():
    lib = L.load()
    a0 = np.arange(8, dtype=np.float32)
    avg, p = dev(a0, 0), dev(a0 + 1, 0)
    st = L.stream_ptr()
    for n, decay, every, step, a, b in ((8, 1.5, 1, 0, avg, p), (8, -0.1, 1, 0, avg, p), (8, float("nan"), 1, 0, avg, p),
                                        (8, 0.9, 0, 0, avg, p), (-1, 0.9, 1, 0, avg, p), (8, 0.9, 1, -1, avg, p),
                                        (8, 0.9, 1, 0, None, p), (8, 0.9, 1, 0, avg, None)):
        assert lib.szn_ema_step(n, L.ptr(a), L.ptr(b), decay, every, step, None, st) != 0
        assert b"ema_step" in lib.szn_last_error()
    assert lib.szn_ema_step(0, None, None, 0.9, 1, 0, None, st) == 0        # n == 0: a successful no-op
    torch.cuda.synchronize()
    assert np.array_equal(avg.cpu().numpy(), a0)


def special(n, seed):
    """random words with NaNs of several payloads, both zeros and both infinities among them"""
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(n).astype(np.float32).view(np.uint32).copy()
    sp = np.array([0x7fc00000, 0x7fc12345, 0xffc00001, 0x7f800001, 0xff9abcde, 0x00000000, 0x80000000, 0x7f800000, 0xff800000,
                   0x00000001, 0x807fffff], dtype=np.uint32)
    idx = rng.permutation(n)[:min(n, sp.size)]
    w[idx] = sp[:idx.size]
    return w.view(np.int32)


@pytest.mark.parametrize("n", SIZES)
def test_swap_is_bit_exact(n):
    a0, b0 = special(n, 2 * n), special(n, 2 * n + 1)
    for oa, ob in OFFSETS:
        a, b = dev(a0, oa), dev(b0, ob)
        L.call("szn_swap_f32", n, L.ptr(a), L.ptr(b), L.stream_ptr())
        assert L.last_kernel() == "swap_kernel"
        assert np.array_equal(a.cpu().numpy(), b0) and np.array_equal(b.cpu().numpy(), a0), (oa, ob)


def test_swap_bad_arguments_leave_the_data_alone():
    lib = L.load()
    n = 64
    x0 = special(n, 5)
    x = dev(x0, 0)
    st = L.stream_ptr()
    for a, b, m in ((x, x, n), (x, x[2:], n - 2), (x[5:], x, n - 5), (x[:32], x[31:], 32)):          # overlapping ranges
        assert lib.szn_swap_f32(m, L.ptr(a), L.ptr(b), st) != 0
        assert b"overlap" in lib.szn_last_error()
    assert lib.szn_swap_f32(-1, L.ptr(x), L.ptr(x[32:]), st) != 0
    assert lib.szn_swap_f32(8, None, L.ptr(x), st) != 0 and lib.szn_swap_f32(8, L.ptr(x), None, st) != 0
    assert lib.szn_swap_f32(0, None, None, st) == 0
    torch.cuda.synchronize()
    assert np.array_equal(x.cpu().numpy(), x0)
    L.call("szn_swap_f32", 32, L.ptr(x[:32]), L.ptr(x[32:]), st)             # adjacent halves do not overlap
    got = x.cpu().numpy()
    assert np.array_equal(got[:32], x0[32:]) and np.array_equal(got[32:], x0[:32])
