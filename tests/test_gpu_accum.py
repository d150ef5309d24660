"""GPU: szn_grad_accum through the C interface, against numpy bit for bit (a float32 addition is correctly rounded: there is no
tolerance; NaNs are compared by position).  Sizes cross the kernel's paths: a lone scalar, less than one vector, one vector, around one
256-thread block, several blocks with a tail, and 2^20 + 5 elements (blocks of vector pairs, lanes with an odd last vector); element
offsets (1, 1) move both pointers off their 16-byte boundary (scalar head + vector body), (0, 1) is the all-scalar path.  All of those
finish in one round of the kernel's loops; test_grid_stride_rounds holds the two sizes past the largest grid."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers_accum as R  # noqa: E402
from zeroshotsemanticsegmentation_amd import _lib as L  # noqa: E402

SIZES = [1, 3, 4, 255, 256, 257, 1023, 4099, 2 ** 20 + 5]
OFFSETS = [(0, 0), (1, 1), (0, 1)]
MODES = [L.ACCUM_SET, L.ACCUM_ADD, L.ACCUM_FINAL]


def dev(a, off):
    """`a` on the GPU behind `off` spare elements: off = 1 puts it 4 bytes past a 16-byte boundary"""
    base = torch.empty(a.size + off, dtype=torch.float32, device="cuda")
    assert base.data_ptr() % 16 == 0
    t = base[off:]
    t.copy_(torch.from_numpy(a))
    return t


def accum(acc, grad, mode):
    L.call("szn_grad_accum", grad.numel(), L.ptr(acc), L.ptr(grad), mode, L.stream_ptr())


def bits(t):
    return t.view(torch.int32).cpu().numpy().copy()


@pytest.mark.parametrize("n", SIZES)
def test_three_modes_bit_for_bit(n):
    a0, g0 = R.special_pair(n, n)
    want = R.accumulate([a0, g0])
    for oa, og in OFFSETS:
        # SET: acc becomes grad's bits (payloads included: a copy), grad is only read
        acc, grad = dev(a0, oa), dev(g0, og)
        accum(acc, grad, L.ACCUM_SET)
        assert L.last_kernel() == "grad_accum_kernel"
        assert np.array_equal(bits(acc), g0.view(np.int32)) and np.array_equal(bits(grad), g0.view(np.int32)), (oa, og)
        # ADD: acc = acc + grad, grad is only read
        acc, grad = dev(a0, oa), dev(g0, og)
        accum(acc, grad, L.ACCUM_ADD)
        assert R.same_floats(acc.cpu().numpy(), want) and np.array_equal(bits(grad), g0.view(np.int32)), (oa, og)
        # FINAL: grad = acc + grad, acc is only read
        acc, grad = dev(a0, oa), dev(g0, og)
        accum(acc, grad, L.ACCUM_FINAL)
        assert R.same_floats(grad.cpu().numpy(), want) and np.array_equal(bits(acc), a0.view(np.int32)), (oa, og)
    if n >= 255:
        assert int((want.astype(np.float64) != a0.astype(np.float64) + g0.astype(np.float64)).sum()) > 0      # additions really round


@pytest.mark.parametrize("n,off", [(257, (0, 0)), (4099, (1, 1)), (4099, (0, 1)), (2 ** 20 + 5, (0, 0))])
def test_window_is_the_left_to_right_sum(n, off):
    g1, g2 = R.special_pair(n, 3 * n)
    g3 = R.mixed_values(n, 3 * n + 2)
    want = R.accumulate([g1, g2, g3])
    acc = dev(np.full(n, np.nan, np.float32), off[0])                        # SET must not read what the accumulator held
    grad = dev(g1, off[1])
    accum(acc, grad, L.ACCUM_SET)
    grad.copy_(torch.from_numpy(g2))
    accum(acc, grad, L.ACCUM_ADD)
    grad.copy_(torch.from_numpy(g3))
    accum(acc, grad, L.ACCUM_FINAL)
    assert R.same_floats(grad.cpu().numpy(), want)
    assert R.same_floats(acc.cpu().numpy(), R.accumulate([g1, g2]))
    other = R.accumulate([g3, g2, g1])
    if n >= 4099:
        assert not R.same_floats(want, other)                                # the order matters on these inputs
    # two windows give the same bits
    acc2, grad2 = dev(g1, off[0]), dev(g1, off[1])
    accum(acc2, grad2, L.ACCUM_SET)
    grad2.copy_(torch.from_numpy(g2))
    accum(acc2, grad2, L.ACCUM_ADD)
    grad2.copy_(torch.from_numpy(g3))
    accum(acc2, grad2, L.ACCUM_FINAL)
    assert np.array_equal(bits(grad2), bits(grad))


GRID = (1 << 17) * 256          # lanes of the largest grid (blocks of 256): beyond it the kernel takes further rounds


@pytest.mark.parametrize("n,off", [(12 * GRID + 2 ** 22 + 5, (0, 0)),        # vectors: a second round of pairs, then odd last vectors
                                   (GRID + 2 ** 20 + 5, (0, 1))],            # all-scalar: a second round of the scalar loop
                         ids=["vector-rounds", "scalar-rounds"])
def test_grid_stride_rounds(n, off):
    """the sizes at which a lane takes more than one round (the 135 M-element weight buffer is one round); reference and comparison on
    the device"""
    g = torch.Generator(device="cuda").manual_seed(n % 1000)
    base_a, base_g = (torch.randn(n + 1, device="cuda", generator=g) for _ in range(2))
    acc, grad = base_a[off[0]:off[0] + n], base_g[off[1]:off[1] + n]
    acc.mul_(1024.0)                                                          # different exponents: the additions round
    grad[::7919] = float("inf")
    a0, g0 = acc.clone(), grad.clone()
    want = a0 + g0
    accum(acc, grad, L.ACCUM_ADD)
    assert torch.equal(acc.view(torch.int32), want.view(torch.int32)) and torch.equal(grad.view(torch.int32), g0.view(torch.int32))
    acc.copy_(a0)
    accum(acc, grad, L.ACCUM_FINAL)
    assert torch.equal(grad.view(torch.int32), want.view(torch.int32)) and torch.equal(acc.view(torch.int32), a0.view(torch.int32))
    del want
    accum(acc, grad, L.ACCUM_SET)
    assert torch.equal(acc.view(torch.int32), grad.view(torch.int32))


def test_bad_arguments_leave_the_data_alone():
    lib = L.load()
    n = 64
    x0 = R.mixed_values(n, 5)
    x = dev(x0, 0)
    y0 = R.mixed_values(n, 6)
    y = dev(y0, 0)
    st = L.stream_ptr()
    for mode in MODES:
        for a, b, m in ((x, x, n), (x, x[2:], n - 2), (x[5:], x, n - 5), (x[:32], x[31:], 32)):          # overlapping ranges
            assert lib.szn_grad_accum(m, L.ptr(a), L.ptr(b), mode, st) == -1
            assert b"overlap" in lib.szn_last_error()
        assert lib.szn_grad_accum(-1, L.ptr(x), L.ptr(y), mode, st) == -1
        assert lib.szn_grad_accum(8, None, L.ptr(y), mode, st) == -1 and lib.szn_grad_accum(8, L.ptr(x), None, mode, st) == -1
        for a, b in ((x.data_ptr() + 2, y.data_ptr()), (x.data_ptr(), y.data_ptr() + 1)):                # not 4-byte aligned
            assert lib.szn_grad_accum(8, a, b, mode, st) == -1
            assert b"aligned" in lib.szn_last_error()
        assert lib.szn_grad_accum(0, None, None, mode, st) == 0                                           # n == 0: a successful no-op
        assert lib.szn_grad_accum(0, L.ptr(x), L.ptr(y), mode, st) == 0
    for mode in (-1, 3, 7):
        assert lib.szn_grad_accum(n, L.ptr(x), L.ptr(y), mode, st) == -1
        assert b"mode" in lib.szn_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(bits(x), x0.view(np.int32)) and np.array_equal(bits(y), y0.view(np.int32))
    accum(x[:32], x[32:], L.ACCUM_ADD)                                       # adjacent halves do not overlap
    got = x.cpu().numpy()
    assert R.same_floats(got[:32], R.accumulate([x0[:32], x0[32:]])) and np.array_equal(got[32:], x0[32:])
