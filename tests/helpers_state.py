"""float64 references for the kernels that own the training state (optimizer steps, loss scale, Dropout2d factors), in plain numpy.

Used by tests/test_state_refs.py (CPU: ties the references to torch.optim and shows that an op-by-op float32 restatement stays inside
the gates) and by tests/test_gpu_state_kernels.py (MI355X: the kernels against the references).  Nothing here touches a GPU.

The C interface takes its hyper-parameters as `float`, so every reference rounds them to float32 FIRST and then works in float64:
`adam_ref(..., b2=0.999)` uses the double value of float32(0.999) everywhere, the bias correction included.  (torch.optim.Adam with the
literal 0.999 uses the Python double there; tests/test_state_refs.py states that distance as a number.)
"""
import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24                     # unit round-off of float32
FLOOR = 2.0 ** -126                # smallest normal float32: absolute floor of the moment bounds (denormal handling is not in the contract)

ADAM_STEPS = (1, 2, 10, 1000, 100000)
ADAM_WDS = (0.0, 0.01)
GRAD_SCALES = (1.0, 1.0 / 64, 1.0 / 32768)
SGD_MOMENTUM = 0.99
SGD_WDS = (0.0, 5e-4)
SIZES = (1, 3, 4, 5, 255, 1023, 2 ** 20 + 3)
ADAM_HP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)
SGD_LR = 1e-2


def f32v(x):
    """the double value of float32(x): what a `float` argument of the C interface carries"""
    return float(F32(x))


# ---- optimizer chains ---------------------------------------------------------------------------------------------------------
def _scaled_grad64(p, g, wd, grad_scale, loss_scale):
    g = np.asarray(g, F64) * (f32v(grad_scale) / f32v(loss_scale))
    wd = f32v(wd)
    if wd != 0.0:
        g = g + wd * np.asarray(p, F64)
    return g


def adam_ref(p, g, m, v, lr, b1, b2, eps, wd, step, grad_scale=1.0, loss_scale=1.0):
    """torch.optim.Adam (no amsgrad), float64: g' = g * grad_scale / loss_scale (+ wd p); m, v; bias corrections from `step`; update.
    Returns (p, m, v)."""
    lr, b1, b2, eps = f32v(lr), f32v(b1), f32v(b2), f32v(eps)
    p, m, v = np.asarray(p, F64), np.asarray(m, F64), np.asarray(v, F64)
    g = _scaled_grad64(p, g, wd, grad_scale, loss_scale)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    denom = np.sqrt(v) / np.sqrt(bc2) + eps
    return p - (lr / bc1) * (m / denom), m, v


def sgd_ref(p, g, buf, lr, momentum, wd, first_step, grad_scale=1.0, loss_scale=1.0):
    """torch.optim.SGD (momentum, dampening 0, no nesterov), float64.  first_step: buf = g', the old buffer is not read.
    Returns (p, buf)."""
    lr, momentum = f32v(lr), f32v(momentum)
    p = np.asarray(p, F64)
    g = _scaled_grad64(p, g, wd, grad_scale, loss_scale)
    buf = g.copy() if first_step else momentum * np.asarray(buf, F64) + g
    return p - lr * buf, buf


def adam_scalars_f32(lr, b1, b2, step):
    """szn_adam_scalars: step_size = lr / (1 - b1^t), inv_bc2_sqrt = 1 / sqrt(1 - b2^t), formed in double from the float32 values,
    each rounded once to float32"""
    bc1, bc2 = 1.0 - f32v(b1) ** step, 1.0 - f32v(b2) ** step
    return F32(f32v(lr) / bc1), F32(1.0 / np.sqrt(bc2))


def _scaled_grad32(p, g, wd, grad_scale, loss_scale):
    gs = F32(grad_scale) if loss_scale == 1.0 else F32(grad_scale) / F32(loss_scale)
    g = np.asarray(g, F32) * gs
    wd = F32(wd)
    if wd != 0:                      # one fused multiply-add: exact product and sum in float64, rounded once
        g = (F64(wd) * np.asarray(p, F64) + g.astype(F64)).astype(F32)
    return g


def adam_f32(p, g, m, v, lr, b1, b2, eps, wd, step, grad_scale=1.0, loss_scale=1.0):
    """the chain of adam_ref op by op in float32, every operation rounded once.  Calibrates the gates; it is NOT the reference."""
    p, m, v = np.asarray(p, F32), np.asarray(m, F32), np.asarray(v, F32)
    b1, b2, eps = F32(b1), F32(b2), F32(eps)
    one = F32(1)
    step_size, inv_bc2_sqrt = adam_scalars_f32(lr, b1, b2, step)
    with np.errstate(under="ignore"):
        g = _scaled_grad32(p, g, wd, grad_scale, loss_scale)
        m = b1 * m + (one - b1) * g
        v = b2 * v + ((one - b2) * g) * g
        denom = np.sqrt(v) * inv_bc2_sqrt + eps
        p = p - step_size * (m / denom)
    assert p.dtype == F32 and m.dtype == F32 and v.dtype == F32
    return p, m, v


def sgd_f32(p, g, buf, lr, momentum, wd, first_step, grad_scale=1.0, loss_scale=1.0):
    p = np.asarray(p, F32)
    with np.errstate(under="ignore"):
        g = _scaled_grad32(p, g, wd, grad_scale, loss_scale)
        buf = g.copy() if first_step else F32(momentum) * np.asarray(buf, F32) + g
        p = p - F32(lr) * buf
    assert p.dtype == F32 and buf.dtype == F32
    return p, buf


# ---- gates ---------------------------------------------------------------------------------------------------------------------
def master_units(p_test, p_new64, p_old64):
    """|p_test - p64| in units of ulp32(p64) + 2^-23 |delta p64|, per element"""
    unit = np.spacing(np.abs(p_new64).astype(F32)).astype(F64) + 2.0 ** -23 * np.abs(p_new64 - np.asarray(p_old64, F64))
    return np.abs(np.asarray(p_test, F64) - p_new64) / unit


def master_gate(restatement_units):
    """c of the master gate: twice the float32 restatement's own worst error on the same inputs, plus 1"""
    return 2.0 * float(np.max(restatement_units)) + 1.0


def grad_magnitude(p, g, wd, grad_scale=1.0, loss_scale=1.0):
    """G = |g grad_scale / loss_scale| + |wd p|: the magnitude the rounding errors of g' are relative to.  Without weight decay G = |g'|.
    With it, g' = wd p + g s may cancel, and its error stays relative to the operands: |fl(g s) - g s| <= u |g s|, then one fma rounding
    u |g'|, so |g'_32 - g'| <= 2 u G (first order)."""
    return np.abs(np.asarray(g, F64) * (f32v(grad_scale) / f32v(loss_scale))) + np.abs(f32v(wd) * np.asarray(p, F64))


def adam_moment_bounds(p, g, m, v, b1, b2, wd, grad_scale=1.0, loss_scale=1.0):
    """one-step bounds of the float32 moments against adam_ref's (u = 2^-24, first order, G = grad_magnitude):
        m: error of g' 2 u G, product (1-b1) g' +u -> 3 u (1-b1) G; product b1 m: u |b1 m|; the sum: u (|b1 m| + (1-b1) G)
           => 2 u |b1 m| + 4 u (1-b1) G  <=  6 u (|b1 m| + (1-b1) G)
        v: ((1-b2) g') g': 3 u + 2 u + u = 6 u (1-b2) G^2; product b2 v: u b2 v; the sum: u (b2 v + (1-b2) G^2)
           => 2 u b2 v + 7 u (1-b2) G^2  <=  8 u (b2 v + (1-b2) G^2)
    each with the absolute floor 2^-126 (products that underflow lose at most 2^-149 each)."""
    b1, b2 = f32v(b1), f32v(b2)
    G = grad_magnitude(p, g, wd, grad_scale, loss_scale)
    bm = 6 * U * (np.abs(b1 * np.asarray(m, F64)) + (1.0 - b1) * G) + FLOOR
    bv = 8 * U * (b2 * np.asarray(v, F64) + (1.0 - b2) * G * G) + FLOOR
    return bm, bv


def sgd_buf_bound(p, g, buf, momentum, wd, first_step, grad_scale=1.0, loss_scale=1.0):
    """buf = mom buf + g': error of g' 2 u G, product u |mom buf|, the sum u (|mom buf| + G)  =>  <= 4 u (|mom buf| + G), floor 2^-126.
    On the first step buf = g' and the old buffer does not enter."""
    G = grad_magnitude(p, g, wd, grad_scale, loss_scale)
    old = 0.0 if first_step else np.abs(f32v(momentum) * np.asarray(buf, F64))
    return 4 * U * (old + G) + FLOOR


# ---- the inputs of the optimizer tests -------------------------------------------------------------------------------------------
def opt_inputs(n, seed):
    """weights ~ N(0, 0.02); gradients log-normal over 1e-12 .. 1e2 with both signs, a block of exact zeros, a block of +-1e-23 (g^2
    underflows); moments / momentum buffer from a previous step on another such gradient; a block with g = m = v = buf = 0 (`zero`).
    If n % 4 != 0 the last n % 4 elements repeat the first ones: the scalar tail then sees values that the vector body also sees."""
    rng = np.random.default_rng(seed)

    def lognormal():
        return (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-12, 2, n)).astype(F32)
    p = (rng.standard_normal(n) * 0.02).astype(F32)
    g, gp = lognormal(), lognormal()
    zero = np.zeros(n, bool)
    if n >= 16:
        w = max(1, n // 16)
        g[n // 8:n // 8 + w] = 0.0
        g[n // 4:n // 4 + w] = (rng.choice([-1.0, 1.0], w) * 1e-23).astype(F32)
        zero[n // 2:n // 2 + w] = True
    elif n >= 3:
        zero[1] = True
        g[2] = 1e-23
    m = (F64(1.0 - f32v(0.9)) * gp).astype(F32)
    v = (F64(1.0 - f32v(0.999)) * gp.astype(F64) ** 2).astype(F32)
    buf = gp.copy()
    for a in (g, m, v, buf):
        a[zero] = 0.0
    r = n % 4
    if r and n > 4:
        for a in (p, g, m, v, buf, zero):
            a[n - r:] = a[:r]
    return dict(p=p, g=g, m=m, v=v, buf=buf, zero=zero)


# ---- loss scale -------------------------------------------------------------------------------------------------------------------
def loss_scale_model(state, growth, backoff, interval, lo, hi):
    """szn_loss_scale_update on four float32 words {S, found_inf, steps applied, clean steps since S last changed}, from the contract
    in include/szn.h: after an overflow S backs off (x backoff, not below lo), the clean count restarts and no step is counted;
    otherwise the step is counted, and after `interval` clean steps S grows (x growth, not above hi, and growth never LOWERS S: a
    scale that already stands at or above hi stays) and the clean count restarts.  The flag is cleared either way."""
    S, flag, steps, clean = (F32(x) for x in state)
    growth, backoff, lo, hi = F32(growth), F32(backoff), F32(lo), F32(hi)
    if flag != 0:
        S = max(S * backoff, lo)
        clean = F32(0)
    else:
        steps = steps + F32(1)
        clean = clean + F32(1)
        if clean >= F32(interval):
            S = max(S, min(S * growth, hi))
            clean = F32(0)
    return np.array([S, 0.0, steps, clean], F32)


# ---- Dropout2d factors ------------------------------------------------------------------------------------------------------------
_M64 = (1 << 64) - 1


def dropout_ref(n, p, seed, offset):
    """the counter-based generator: splitmix64(seed * 0xD1342543DE82EF95 + offset + i), top 24 bits as a uniform in [0, 1), keep where
    u >= p, kept value float32(1) / (float32(1) - float32(p))"""
    base = ((int(seed) & _M64) * 0xD1342543DE82EF95 + (int(offset) & _M64)) & _M64
    with np.errstate(over="ignore"):
        z = np.uint64(base) + np.arange(n, dtype=np.uint64)
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    u = (z >> np.uint64(40)).astype(F32) * F32(2.0 ** -24)
    keep = F32(1) / (F32(1) - F32(p))
    return np.where(u >= F32(p), keep, F32(0)).astype(F32)
