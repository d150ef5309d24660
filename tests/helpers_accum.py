"""The reference of gradient accumulation, in plain numpy: the left-to-right float32 sum ((g1 + g2) + g3) + ... + gA -- the order torch
gives `.grad` when backward() runs A times without zero_grad(), and the order SZN_ACCUM_SET, _ADD ..., _FINAL produce -- and its mean.

Used by tests/test_accum_ref.py (CPU: ties it to torch's idiom and to the float64 optimizer references of tests/helpers_state.py) and
by the GPU tests of szn_grad_accum.  Nothing here touches a GPU."""
import numpy as np

F32 = np.float32


def accumulate(grads, average=False):
    """grads: a sequence of float32 arrays of one shape -> their sum, added left to right with one float32 rounding per addition;
    average: divided by len(grads) in float32 afterwards (one more rounding)"""
    grads = [np.asarray(g) for g in grads]
    assert grads and all(g.dtype == F32 and g.shape == grads[0].shape for g in grads)
    with np.errstate(invalid="ignore", over="ignore"):       # inf + -inf = nan is part of the contract
        s = grads[0].copy()
        for g in grads[1:]:
            s = s + g
        if average:
            s = s / F32(len(grads))
    assert s.dtype == F32
    return s


def mixed_values(n, seed, specials=True):
    """float32 test values for an exact-sum test: mixed signs, exponents spread over about +-20 (so that additions really round), no
    subnormals; with `specials` a few inf, -inf, nan and -0.0 elements at fixed relative positions (see special_pair)"""
    rng = np.random.default_rng(seed)
    x = (rng.choice([-1.0, 1.0], n) * rng.uniform(1.0, 2.0, n) * 2.0 ** rng.integers(-20, 21, n)).astype(F32)
    assert np.all(np.abs(x) >= 2.0 ** -21)
    if specials and n >= 8:
        for k, v in enumerate((np.inf, -np.inf, np.nan, -0.0)):
            x[(seed + 3 * k) % n] = v
    return x


def special_pair(n, seed):
    """two arrays of mixed_values whose special elements meet: inf + -inf, inf + inf, nan + finite, -0.0 + -0.0, -0.0 + 0.0, x + -x"""
    a, b = mixed_values(n, seed), mixed_values(n, seed + 1000)
    if n >= 8:
        i = np.arange(6) * (n // 8) + 1
        a[i] = np.array([np.inf, np.inf, np.nan, -0.0, -0.0, 3.5], F32)
        b[i] = np.array([-np.inf, np.inf, 1.0, -0.0, 0.0, -3.5], F32)
    return a, b


def same_floats(got, want):
    """bit for bit, except that NaNs are compared by position (payloads are not part of the contract)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == F32 and want.dtype == F32 and got.shape == want.shape
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan]))
