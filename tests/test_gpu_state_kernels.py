"""The kernels that own the training state, each called through the C interface and compared with a float64 reference of the same
operation (tests/helpers_state.py): szn_adam_step / szn_sgd_momentum_step, their _g16 and _scaled forms, szn_grad_check_finite,
szn_loss_scale_update, szn_cast and szn_dropout2d_mask.

Gates (none of their numbers comes from a kernel):
* master weights: |p_gpu - p64| <= c (ulp32(p64) + 2^-23 |dp64|) per element, c = 2 x (the worst error, in that unit, of the numpy
  float32 restatement of the chain on the same inputs) + 1.  The kernel's division and square root are correctly rounded and the
  build forbids contraction, so the restatement is the kernel's arithmetic up to where the one fma sits.
* Adam moments: |m - m64| <= 6 u (|b1 m| + (1-b1) G) and |v - v64| <= 8 u (b2 v + (1-b2) G^2), u = 2^-24, G = |g s| + |wd p| (= |g'|
  without weight decay), each with the floor 2^-126; SGD's buffer: 4 u (|mom buf| + G).  Derivations: helpers_state.adam_moment_bounds /
  sgd_buf_bound; tests/test_state_refs.py shows that the float32 restatement fits them.
* the 16-bit weight image equals torch's CPU round-to-nearest-even conversion of the kernel's OWN new master, bit for bit, in the
  16-byte vector body (v_cvt_pk_*) and in the scalar tail / unaligned path.
* loss scale, casts, Dropout2d factors, the overflow flag: exact equality with a CPU computation.
Every buffer is a view into a larger allocation filled with a sentinel pattern: the elements before and after the view must come back
untouched.  Non-finite values below are DATA for kernels that are specified on them; nothing here provokes a fault.
"""
import ctypes as C
import functools
import itertools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from zeroshotsemanticsegmentation_amd import _lib as L  # noqa: E402
import helpers_state as H  # noqa: E402

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
PAD = 8                                  # guard elements on either side of a view (the view of offset 0 stays 16-byte aligned)
SENT = {4: 0x7FA5A5A5, 2: 0x7FA5}        # sentinel bit patterns (NaNs: a kernel that reads a guard element shows it)
HP = H.ADAM_HP
INF, NAN = float("inf"), float("nan")


class Buf:
    """n elements of `dtype` at element offset PAD + off of a sentinel-filled device allocation"""

    def __init__(self, values, dtype, off=0, n=None):
        self.dtype, self.size = dtype, torch.empty(0, dtype=dtype).element_size()
        if values is not None:
            values = values if torch.is_tensor(values) else torch.from_numpy(np.ascontiguousarray(values))
            n = values.numel()
        self.n, self.lo = n, PAD + off
        it = torch.int32 if self.size == 4 else torch.int16
        self.raw = torch.full((self.lo + n + PAD,), SENT[self.size], dtype=it, device="cuda")
        self.t = self.raw.view(dtype)[self.lo:self.lo + n]
        if values is not None:
            self.t.copy_(values.to(dtype))
        self.ptr = C.c_void_p(self.t.data_ptr())
        assert self.t.data_ptr() % 16 == (off * self.size) % 16

    def bits(self):
        return self.raw[self.lo:self.lo + self.n].cpu().numpy()

    def np(self):
        return self.t.float().cpu().numpy()

    def guards_ok(self):
        s = SENT[self.size]
        return bool((self.raw[:self.lo] == s).all()) and bool((self.raw[self.lo + self.n:] == s).all())


def fbits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def rne_bits(a32, lp):
    """torch's CPU round-to-nearest-even conversion of float32 values, as 16-bit patterns"""
    return torch.from_numpy(np.ascontiguousarray(a32, np.float32)).to(lp).view(torch.int16).numpy()


# (state offset, gradient offset, weight-image offset) in elements
LAYOUTS = {"aligned": (0, 0, 0), "all+1": (1, 1, 1), "all+2": (2, 2, 2), "all+3": (3, 3, 3), "grad+1": (0, 1, 0), "wlp+1": (0, 0, 1)}
GTYPES = [F32, BF16, F16]
ADAM_COMBOS = list(itertools.product(H.ADAM_STEPS, H.ADAM_WDS, H.GRAD_SCALES))                      # 30
SGD_COMBOS = list(itertools.product((1, 0), H.SGD_WDS, (H.SGD_LR, 2 * H.SGD_LR)))                  # 8
CASES = [(lay, gt) for lay in LAYOUTS for gt in GTYPES]                                            # 18
BIG = H.SIZES[-1]


@functools.lru_cache(maxsize=4)
def inputs(n):
    return H.opt_inputs(n, seed=n)


def gradient(x, gtype):
    """(the tensor the kernel reads, its widened float32 values)"""
    g = torch.from_numpy(x["g"])
    if gtype == F32:
        return g, x["g"]
    g16 = g.to(gtype)
    return g16, g16.float().numpy()


def lp_for(layout, i):
    return (BF16, F16)[i % 2] if layout == "wlp+1" else (BF16, F16, None)[i % 3]


def tail_repeats_head(n, layout, arrays):
    """aligned buffers: the last n % 4 elements (scalar tail) got the inputs of the first ones (vector body): same outputs, bit for bit"""
    r = n % 4
    if layout == "aligned" and r and n > 4:
        for a in arrays:
            if a is not None:
                assert np.array_equal(a[n - r:], a[:r])


def adam_run(x, layout, gtype, lp, wd, step, gs, dyn=None, S=1.0):
    """one Adam step on the GPU from the state in x, checked against adam_ref.  dyn: a Buf {S, 0, t, clean} -> szn_adam_step_scaled
    (then step must be t + 1 and S the scale).  Returns (p, m, v, worst error in units, c)."""
    n = len(x["p"])
    so, go, wo = LAYOUTS[layout]
    gt, gw = gradient(x, gtype)
    P, M, V, G = Buf(x["p"], F32, so), Buf(x["m"], F32, so), Buf(x["v"], F32, so), Buf(gt, gtype, go)
    W = Buf(None, lp, wo, n=n) if lp is not None else None
    bystander = Buf(None, BF16, 0, n=min(n, 64))
    g_before = G.bits()
    wp, wc, st = (W.ptr if W else None), (L.dtype_code(lp) if lp is not None else 7), L.stream_ptr()
    if dyn is not None:
        assert gtype == F32
        L.call("szn_adam_step_scaled", n, P.ptr, G.ptr, M.ptr, V.ptr, HP["lr"], HP["b1"], HP["b2"], HP["eps"], wd, dyn.ptr, gs, wp, wc, st)
    elif gtype == F32:
        L.call("szn_adam_step", n, P.ptr, G.ptr, M.ptr, V.ptr, HP["lr"], HP["b1"], HP["b2"], HP["eps"], wd, step, gs, wp, wc, st)
    else:
        L.call("szn_adam_step_g16", n, P.ptr, G.ptr, L.dtype_code(gtype), M.ptr, V.ptr, HP["lr"], HP["b1"], HP["b2"], HP["eps"], wd,
               step, gs, wp, wc, st)
    assert L.last_kernel() == ("adam_kernel" if gtype == F32 else "adam_kernel_g16")
    torch.cuda.synchronize()
    for b in (P, M, V, G, W, bystander):
        assert b is None or b.guards_ok()
    assert np.array_equal(G.bits(), g_before)
    assert bool((bystander.raw == SENT[2]).all())              # (w_lp = NULL: no image is written anywhere)
    p, m, v = P.np(), M.np(), V.np()
    a = (x["p"], gw, x["m"], x["v"], HP["lr"], HP["b1"], HP["b2"], HP["eps"], wd, step, gs, S)
    p64, m64, v64 = H.adam_ref(*a)
    c = H.master_gate(H.master_units(H.adam_f32(*a)[0], p64, x["p"]))
    units = H.master_units(p, p64, x["p"])
    what = (n, layout, gtype, lp, wd, step, gs, S)
    assert units.max() <= c, (what, float(units.max()), c, int(units.argmax()))
    bm, bv = H.adam_moment_bounds(x["p"], gw, x["m"], x["v"], HP["b1"], HP["b2"], wd, gs, S)
    assert np.all(np.abs(m - m64) <= bm), what
    assert np.all(np.abs(v - v64) <= bv), what
    if wd == 0.0:                                              # g = m = v = 0: the master comes back bit-identical
        assert np.array_equal(fbits(p)[x["zero"]], fbits(x["p"])[x["zero"]]), what
    wbits = None
    if W is not None:
        wbits = W.bits()
        assert np.array_equal(wbits, rne_bits(p, lp)), what
    tail_repeats_head(n, layout, (fbits(p), fbits(m), fbits(v), wbits))
    return p, m, v, float(units.max()), c


def sgd_run(x, layout, gtype, lp, wd, first, lr, gs=1.0, dyn=None, S=1.0):
    n = len(x["p"])
    so, go, wo = LAYOUTS[layout]
    gt, gw = gradient(x, gtype)
    buf0 = np.full(n, np.nan, np.float32) if first else x["buf"]          # first step: the buffer holds NaN and must not be read
    P, B, G = Buf(x["p"], F32, so), Buf(buf0, F32, so), Buf(gt, gtype, go)
    W = Buf(None, lp, wo, n=n) if lp is not None else None
    g_before = G.bits()
    wp, wc, st = (W.ptr if W else None), (L.dtype_code(lp) if lp is not None else 7), L.stream_ptr()
    mom = H.SGD_MOMENTUM
    if dyn is not None:
        assert gtype == F32
        L.call("szn_sgd_momentum_step_scaled", n, P.ptr, G.ptr, B.ptr, lr, mom, wd, dyn.ptr, gs, wp, wc, st)
    elif gtype == F32:
        L.call("szn_sgd_momentum_step", n, P.ptr, G.ptr, B.ptr, lr, mom, wd, first, gs, wp, wc, st)
    else:
        L.call("szn_sgd_momentum_step_g16", n, P.ptr, G.ptr, L.dtype_code(gtype), B.ptr, lr, mom, wd, first, gs, wp, wc, st)
    assert L.last_kernel() == ("sgd_kernel" if gtype == F32 else "sgd_kernel_g16")
    torch.cuda.synchronize()
    for b in (P, B, G, W):
        assert b is None or b.guards_ok()
    assert np.array_equal(G.bits(), g_before)
    p, buf = P.np(), B.np()
    what = (n, layout, gtype, lp, wd, first, lr, gs, S)
    assert np.all(np.isfinite(p)) and np.all(np.isfinite(buf)), what
    a = (x["p"], gw, buf0, lr, mom, wd, first, gs, S)
    p64, b64 = H.sgd_ref(*a)
    c = H.master_gate(H.master_units(H.sgd_f32(*a)[0], p64, x["p"]))
    units = H.master_units(p, p64, x["p"])
    assert units.max() <= c, (what, float(units.max()), c, int(units.argmax()))
    assert np.all(np.abs(buf - b64) <= H.sgd_buf_bound(x["p"], gw, buf0, mom, wd, first, gs, S)), what
    if first and wd == 0.0 and gs == 1.0 and S == 1.0:         # buf == g': one exact copy
        assert np.array_equal(fbits(buf), fbits(gw)), what
    wbits = None
    if W is not None:
        wbits = W.bits()
        assert np.array_equal(wbits, rne_bits(p, lp)), what
    tail_repeats_head(n, layout, (fbits(p), fbits(buf), wbits))
    return p, buf, float(units.max()), c


# ---- 1. optimizer steps against float64 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,gtype", CASES)
def test_adam_step_against_float64_small_sizes(layout, gtype):
    worst = cmax = 0.0
    for n in H.SIZES[:-1]:
        for i, (step, wd, gs) in enumerate(ADAM_COMBOS):
            _, _, _, u, c = adam_run(inputs(n), layout, gtype, lp_for(layout, i + n), wd, step, gs)
            worst, cmax = max(worst, u), max(cmax, c)
    print("adam %s %s: worst master error %.2f units, largest gate c %.2f" % (layout, gtype, worst, cmax))


@pytest.mark.parametrize("k,case", list(enumerate(CASES)))
def test_adam_step_against_float64_large(k, case):
    """n = 2^20 + 3: the 18 (layout, gradient type) cases share out the 30 hyper-parameter combinations, two each"""
    layout, gtype = case
    for i in (2 * k, 2 * k + 1):
        step, wd, gs = ADAM_COMBOS[i % len(ADAM_COMBOS)]
        _, _, _, u, c = adam_run(inputs(BIG), layout, gtype, lp_for(layout, i), wd, step, gs)
        print("adam n=%d %s %s step %d wd %g gs %g: master error %.2f units, gate c %.2f" % (BIG, layout, gtype, step, wd, gs, u, c))


@pytest.mark.parametrize("layout,gtype", CASES)
def test_sgd_step_against_float64_small_sizes(layout, gtype):
    worst = cmax = 0.0
    for n in H.SIZES[:-1]:
        for i, (first, wd, lr) in enumerate(SGD_COMBOS):
            _, _, u, c = sgd_run(inputs(n), layout, gtype, lp_for(layout, i + n), wd, first, lr)
            worst, cmax = max(worst, u), max(cmax, c)
    print("sgd %s %s: worst master error %.2f units, largest gate c %.2f" % (layout, gtype, worst, cmax))


@pytest.mark.parametrize("k,case", list(enumerate(CASES)))
def test_sgd_step_against_float64_large(k, case):
    layout, gtype = case
    for i in (2 * k, 2 * k + 1):
        first, wd, lr = SGD_COMBOS[i % len(SGD_COMBOS)]
        _, _, u, c = sgd_run(inputs(BIG), layout, gtype, lp_for(layout, i), wd, first, lr)
        print("sgd n=%d %s %s first %d wd %g lr %g: master error %.2f units, gate c %.2f" % (BIG, layout, gtype, first, wd, lr, u, c))


@pytest.mark.parametrize("layout", ["aligned", "all+1"])
def test_five_chained_steps_each_checked_from_the_gpu_state(layout):
    """every step starts from the state the GPU produced in the step before, so the bounds stay one-step bounds"""
    n = 4099
    rng = np.random.default_rng(11)
    xa = {k: v.copy() for k, v in H.opt_inputs(n, seed=5).items()}
    xs = {k: v.copy() for k, v in xa.items()}
    p_start = xa["p"].copy()
    for t in range(1, 6):
        g = (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-6, 0, n)).astype(np.float32)
        g[n - n % 4:] = g[:n % 4]                               # (the tail keeps repeating the head: tail_repeats_head)
        xa["g"] = xs["g"] = g
        xa["zero"] = xs["zero"] = np.zeros(n, bool)
        xa["p"], xa["m"], xa["v"], _, _ = adam_run(xa, layout, F32, BF16, 0.01, t, 1.0 / 64)
        xs["p"], xs["buf"], _, _ = sgd_run(xs, layout, F32, F16, 5e-4, int(t == 1), H.SGD_LR)
    assert np.mean(xa["p"] != p_start) > 0.99 and np.mean(xs["p"] != p_start) > 0.99          # the last master has moved


@pytest.mark.parametrize("lp", [BF16, F16])
def test_weight_image_rounds_the_master_to_nearest_even_in_body_and_tail(lp):
    """a step that moves nothing (g = m = v = 0, no weight decay) on masters that sit ON the 16-bit grid's ties, one float32 ulp beside
    them, at the overflow threshold and among the denormals: the image is torch's conversion of the master, in the vector body
    (v_cvt_pk_*, aligned buffers) and in the scalar path (to_bits16: the tail, and every element of an unaligned slice)"""
    vals = cast_inputs(lp)
    vals = vals[torch.isfinite(vals)].numpy()
    n = (len(vals) - 3) // 4 * 4 + 3
    vals = vals[:n].copy()
    vals[n - 3:] = vals[:3]
    z = np.zeros(n, np.float32)
    want = rne_bits(vals, lp)
    st = L.stream_ptr()
    for off in (0, 1):
        for opt in ("adam", "sgd"):
            P, G, M, V, W = Buf(vals, F32, off), Buf(z, F32, off), Buf(z, F32, off), Buf(z, F32, off), Buf(None, lp, off, n=n)
            if opt == "adam":
                L.call("szn_adam_step", n, P.ptr, G.ptr, M.ptr, V.ptr, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, W.ptr, L.dtype_code(lp), st)
                assert L.last_kernel() == "adam_kernel"
            else:
                L.call("szn_sgd_momentum_step", n, P.ptr, G.ptr, M.ptr, 1e-2, 0.99, 0.0, 0, 1.0, W.ptr, L.dtype_code(lp), st)
                assert L.last_kernel() == "sgd_kernel"
            torch.cuda.synchronize()
            assert np.array_equal(P.bits(), fbits(vals)), (opt, off)
            got = W.bits()
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, (opt, off, bad.size, [(hex(fbits(vals)[i] & 0xffffffff), hex(got[i] & 0xffff), hex(want[i] & 0xffff))
                                                        for i in bad[:8]])
            assert P.guards_ok() and W.guards_ok()


def _opt_state(n=37):
    x = H.opt_inputs(n, seed=2)
    return x, [Buf(x[k], F32) for k in ("p", "g", "m", "v")], Buf(None, BF16, n=n)


def test_optimizer_calls_with_bad_arguments_are_refused_and_touch_nothing():
    n = 37
    x, (P, G, M, V), W = _opt_state(n)
    G16 = Buf(torch.from_numpy(x["g"]).to(BF16), BF16)
    before = [b.raw.clone() for b in (P, G, M, V, W, G16)]
    st, lpc = L.stream_ptr(), L.SZN_BF16
    hp = (1e-3, 0.9, 0.999, 1e-8, 0.01)
    bad_adam = [(0, P.ptr, G.ptr, M.ptr, V.ptr, *hp, 1, 1.0, W.ptr, lpc, st), (-5, P.ptr, G.ptr, M.ptr, V.ptr, *hp, 1, 1.0, W.ptr, lpc, st),
                (n, P.ptr, G.ptr, M.ptr, V.ptr, *hp, 0, 1.0, W.ptr, lpc, st), (n, P.ptr, G.ptr, M.ptr, V.ptr, *hp, -1, 1.0, W.ptr, lpc, st),
                (n, None, G.ptr, M.ptr, V.ptr, *hp, 1, 1.0, W.ptr, lpc, st), (n, P.ptr, None, M.ptr, V.ptr, *hp, 1, 1.0, W.ptr, lpc, st),
                (n, P.ptr, G.ptr, None, V.ptr, *hp, 1, 1.0, W.ptr, lpc, st), (n, P.ptr, G.ptr, M.ptr, None, *hp, 1, 1.0, W.ptr, lpc, st),
                (n, P.ptr, G.ptr, M.ptr, V.ptr, *hp, 1, 1.0, W.ptr, L.SZN_F32, st), (n, P.ptr, G.ptr, M.ptr, V.ptr, *hp, 1, 1.0, W.ptr, 9, st)]
    for a in bad_adam:
        with pytest.raises(L.SznError):
            L.call("szn_adam_step", *a)
    for gd in (L.SZN_F32, 7, -1):                                  # a gradient of an unknown type
        with pytest.raises(L.SznError):
            L.call("szn_adam_step_g16", n, P.ptr, G16.ptr, gd, M.ptr, V.ptr, *hp, 1, 1.0, W.ptr, lpc, st)
        with pytest.raises(L.SznError):
            L.call("szn_sgd_momentum_step_g16", n, P.ptr, G16.ptr, gd, M.ptr, 1e-2, 0.99, 0.0, 0, 1.0, W.ptr, lpc, st)
    with pytest.raises(L.SznError):
        L.call("szn_adam_step_g16", 0, P.ptr, G16.ptr, L.SZN_BF16, M.ptr, V.ptr, *hp, 1, 1.0, W.ptr, lpc, st)
    with pytest.raises(L.SznError):
        L.call("szn_adam_step_scaled", n, P.ptr, G.ptr, M.ptr, V.ptr, *hp, None, 1.0, W.ptr, lpc, st)
    sg = (1e-2, 0.99, 5e-4)
    bad_sgd = [(0, P.ptr, G.ptr, M.ptr, *sg, 0, 1.0, W.ptr, lpc, st), (-1, P.ptr, G.ptr, M.ptr, *sg, 0, 1.0, W.ptr, lpc, st),
               (n, None, G.ptr, M.ptr, *sg, 0, 1.0, W.ptr, lpc, st), (n, P.ptr, None, M.ptr, *sg, 0, 1.0, W.ptr, lpc, st),
               (n, P.ptr, G.ptr, None, *sg, 0, 1.0, W.ptr, lpc, st), (n, P.ptr, G.ptr, M.ptr, *sg, 0, 1.0, W.ptr, L.SZN_F32, st)]
    for a in bad_sgd:
        with pytest.raises(L.SznError):
            L.call("szn_sgd_momentum_step", *a)
    with pytest.raises(L.SznError):
        L.call("szn_sgd_momentum_step_scaled", n, P.ptr, G.ptr, M.ptr, *sg, None, 1.0, W.ptr, lpc, st)
    torch.cuda.synchronize()
    for b, was in zip((P, G, M, V, W, G16), before):
        assert torch.equal(b.raw, was)


# ---- 2. the _scaled forms ----------------------------------------------------------------------------------------------------------
def scale_state(S, flag, t, clean):
    return Buf(np.array([S, flag, t, clean], np.float32), F32)


@pytest.mark.parametrize("t", [0, 1, 999])
@pytest.mark.parametrize("S", [4096.0, 3000.0])
def test_scaled_adam_is_the_unscaled_step_with_the_scale_divided_out(S, t):
    """flag 0, scale S, t steps applied: the float64 step number t + 1 on g grad_scale / S, inside the gates of section 1.  The clean
    count is set to what the step count is NOT (zero / non-zero), so a kernel that reads the wrong word shows."""
    for n, layout, lp, wd in [(1023, "aligned", BF16, 0.01), (1023, "all+1", F16, 0.0), (2 ** 16 + 3, "aligned", F16, 0.01),
                              (5, "all+3", BF16, 0.01)]:
        x = inputs(n) if n in H.SIZES else H.opt_inputs(n, seed=n)
        dyn = scale_state(S, 0.0, t, 3.0 if t == 0 else 0.0)
        was = dyn.raw.clone()
        p, m, v, u, c = adam_run(x, layout, F32, lp, wd, t + 1, 0.5, dyn=dyn, S=S)
        assert torch.equal(dyn.raw, was)                       # the optimizer kernels never write scale_state
        if S == 4096.0:                                        # a power of two: dividing it out of grad_scale is exact
            q, qm, qv, _, _ = adam_run(x, layout, F32, lp, wd, t + 1, 0.5 / S)
            eq = [float(np.mean(fbits(a) == fbits(b))) for a, b in ((p, q), (m, qm), (v, qv))]
            print("adam scaled vs unscaled, n=%d t=%d %s: bit-equal fraction p %.6f m %.6f v %.6f (worst %.2f units, c %.2f)"
                  % (n, t, layout, eq[0], eq[1], eq[2], u, c))


@pytest.mark.parametrize("t", [0, 1, 999])
@pytest.mark.parametrize("S", [4096.0, 3000.0])
def test_scaled_sgd_is_the_unscaled_step_with_the_scale_divided_out(S, t):
    """first step <=> t == 0 (then the NaN in the buffer must not be read), whatever the clean count says"""
    for n, layout, lp, wd in [(1023, "aligned", BF16, 5e-4), (1023, "all+1", F16, 0.0), (2 ** 16 + 3, "aligned", F16, 5e-4),
                              (5, "all+3", BF16, 5e-4)]:
        x = inputs(n) if n in H.SIZES else H.opt_inputs(n, seed=n)
        dyn = scale_state(S, 0.0, t, 3.0 if t == 0 else 0.0)
        was = dyn.raw.clone()
        p, buf, u, c = sgd_run(x, layout, F32, lp, wd, int(t == 0), H.SGD_LR, gs=0.5, dyn=dyn, S=S)
        assert torch.equal(dyn.raw, was)
        if S == 4096.0:
            q, qb, _, _ = sgd_run(x, layout, F32, lp, wd, int(t == 0), H.SGD_LR, gs=0.5 / S)
            print("sgd scaled vs unscaled, n=%d t=%d %s: bit-equal fraction p %.6f buf %.6f (worst %.2f units, c %.2f)"
                  % (n, t, layout, float(np.mean(fbits(p) == fbits(q))), float(np.mean(fbits(buf) == fbits(qb))), u, c))


@pytest.mark.parametrize("lp", [BF16, F16])
@pytest.mark.parametrize("off", [0, 1])
def test_scaled_steps_do_nothing_when_the_overflow_flag_is_set(lp, off):
    n = 1023                                                    # vector body + a 3-element tail when off == 0, all scalar otherwise
    x = inputs(n)
    st = L.stream_ptr()
    img = torch.from_numpy(x["p"]).to(lp)
    for flag in (1.0, 2.5):
        dyn = scale_state(4096.0, flag, 7.0, 2.0)
        P, G, M, V, W = Buf(x["p"], F32, off), Buf(x["g"], F32, off), Buf(x["m"], F32, off), Buf(x["v"], F32, off), Buf(img, lp, off)
        bufs = (P, G, M, V, W, dyn)
        before = [b.raw.clone() for b in bufs]
        L.call("szn_adam_step_scaled", n, P.ptr, G.ptr, M.ptr, V.ptr, 1e-3, 0.9, 0.999, 1e-8, 0.01, dyn.ptr, 1.0, W.ptr, L.dtype_code(lp), st)
        assert L.last_kernel() == "adam_kernel"
        L.call("szn_sgd_momentum_step_scaled", n, P.ptr, G.ptr, M.ptr, 1e-2, 0.99, 5e-4, dyn.ptr, 1.0, W.ptr, L.dtype_code(lp), st)
        assert L.last_kernel() == "sgd_kernel"
        torch.cuda.synchronize()
        for b, was in zip(bufs, before):
            assert torch.equal(b.raw, was)


# ---- 3. szn_grad_check_finite --------------------------------------------------------------------------------------------------------
STATE0 = np.array([4096.0, 0.0, 7.0, 3.0], np.float32)


def finite_flag(view, state, n):
    """reset the state, run the check over view[:n], return the four words (bit patterns) after it"""
    state.t.copy_(torch.from_numpy(STATE0))
    L.call("szn_grad_check_finite", n, C.c_void_p(view.data_ptr()), state.ptr, L.stream_ptr())
    assert L.last_kernel() == "grad_finite_kernel"
    torch.cuda.synchronize()
    assert state.guards_ok()
    return state.bits()


def expect_flag(words, raised):
    want = fbits(STATE0).copy()
    want[1] = fbits(np.array([1.0 if raised else 0.0], np.float32))[0]
    assert np.array_equal(words, want), (words, want)


def plant_positions(n):
    """where kernels of this shape go wrong: first element, the ends of a block's first pass (256 threads x 1 or 4 elements), the first
    element of the grid-stride loop's second lap (8192 blocks), the last 16-byte group, every tail element, the last element"""
    n4 = n // 4
    pos = {0, 255, 256, 1023, 1024, 8192 * 256 - 1, 8192 * 256, 8192 * 1024 - 1, 8192 * 1024, 4 * n4 - 4, 4 * n4 - 1, n - 1}
    pos |= set(range(4 * n4, n))
    return sorted(i for i in pos if 0 <= i < n)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 1023, 2 ** 20 + 3, 8192 * 1024 + 1203])
def test_grad_check_finite_finds_one_planted_value_anywhere(n):
    g = torch.Generator(device="cuda").manual_seed(n % 977)
    data = torch.randn(n + 2, device="cuda", generator=g)
    state = Buf(STATE0, F32)
    m = n
    for off in (0, 1):                                          # 16-byte aligned (vector body + tail) / offset by one element (all scalar)
        view = data[off:off + n + 1]                            # (one more element than the call is told about)
        assert view.data_ptr() % 16 == 4 * off
        expect_flag(finite_flag(view, state, m), False)
        for i in plant_positions(m):
            keep = view[i:i + 1].clone()
            for val in (INF, -INF, NAN):
                view[i:i + 1].fill_(val)
                expect_flag(finite_flag(view, state, m), True)
            view[i:i + 1].copy_(keep)
        expect_flag(finite_flag(view, state, m), False)        # every plant was taken out again
        view[m:m + 1].fill_(NAN)                                # outside the range: not looked at
        expect_flag(finite_flag(view, state, m), False)
        view[m:m + 1].fill_(0.0)


def test_grad_check_finite_on_finite_extremes_opposite_signs_and_a_raised_flag():
    fmax, tiny = float(np.finfo(np.float32).max), float(np.finfo(np.float32).tiny)
    ext = np.array([fmax, -fmax, tiny, -tiny, 1e-45, -1e-45, 5e-39, -5e-39, -0.0, 0.0, fmax, fmax, -fmax, -fmax, 1.0, -1.0], np.float32)
    vals = np.tile(ext, 67)[:1063]                              # 265 vector groups + a 3-element tail
    state = Buf(STATE0, F32)
    for off in (0, 1):
        b = Buf(vals, F32, off)
        expect_flag(finite_flag(b.t, state, b.n), False)
        assert b.guards_ok() and np.array_equal(b.bits(), fbits(vals))
        # +inf and -inf (and NaN beside inf) inside ONE 16-byte group: no sum or difference of the group's elements may hide them
        for pair in ((INF, -INF), (-INF, INF), (INF, NAN), (INF, INF)):
            b.t[20:22].copy_(torch.tensor(pair))
            expect_flag(finite_flag(b.t, state, b.n), True)
            b.t[20:22].copy_(torch.from_numpy(vals[20:22]))
        # a flag that is already raised stays raised on finite data
        state.t.copy_(torch.from_numpy(np.array([4096.0, 1.0, 7.0, 3.0], np.float32)))
        L.call("szn_grad_check_finite", b.n, b.ptr, state.ptr, L.stream_ptr())
        torch.cuda.synchronize()
        expect_flag(state.bits(), True)
    for a in ((0, b.ptr, state.ptr), (-1, b.ptr, state.ptr), (b.n, None, state.ptr), (b.n, b.ptr, None)):
        with pytest.raises(L.SznError):
            L.call("szn_grad_check_finite", *a, L.stream_ptr())


# ---- 4. szn_loss_scale_update ----------------------------------------------------------------------------------------------------------
H32 = 2.0 ** 32
SCALE_CASES = {                     # (growth, backoff, interval, lo, hi), start state, overflow probability
    "interval1": ((2.0, 0.5, 1, 1.0, H32), (4096.0, 0, 0, 0), 0.3),
    "interval3": ((2.0, 0.5, 3, 1.0, H32), (4096.0, 0, 0, 0), 0.2),
    "interval2000": ((2.0, 0.5, 2000, 1.0, H32), (4096.0, 0, 0, 0), 0.1),
    "not_powers_of_two": ((1.5, 0.7, 4, 1.0, H32), (1000.0, 0, 0, 0), 0.2),
    "floor_holds": ((2.0, 0.5, 2, 1.0, H32), (1.0, 0, 0, 0), 1.0),
    "ceiling_holds": ((2.0, 0.5, 1, 1.0, H32), (H32, 0, 0, 0), 0.0),
    # include/szn.h: growth never lowers S -- a scale that starts above max_scale stays until an overflow backs it off
    "above_ceiling": ((2.0, 0.5, 2, 1.0, H32), (2.0 ** 34, 0, 0, 0), 0.1),
    "trainstep_cosine": ((2.0, 0.5, 2000, 1.0, H32), (4096.0, 0, 5000, 1999), 0.01),        # engine.TrainStep.scale_cfg, growth in reach
    "trainstep_ce": ((2.0, 0.5, 2000, 2.0 ** -8, H32), (1.0, 0, 5000, 1995), 0.6),           # the CE heads' floor 2^-8
}


@pytest.mark.parametrize("name", list(SCALE_CASES))
def test_loss_scale_update_follows_the_model_word_for_word(name):
    cfg, start, p_over = SCALE_CASES[name]
    rng = np.random.default_rng(len(name) * 101 + 7)
    model = np.array(start, np.float32)
    state = Buf(model, F32)
    st = L.stream_ptr()
    seen = set()
    for k in range(200):
        over = bool(rng.random() < p_over)
        if over:
            state.t[1:2].fill_(1.0)
            model[1] = 1.0
        before = float(model[0])
        L.call("szn_loss_scale_update", state.ptr, *cfg, st)
        assert L.last_kernel() == "loss_scale_update_kernel"
        model = H.loss_scale_model(model, *cfg)
        torch.cuda.synchronize()
        assert np.array_equal(state.bits(), fbits(model)), (name, k, over, state.np(), model)
        seen.add("down" if model[0] < before else "up" if model[0] > before else "same")
        assert over or model[0] >= before                       # growth never lowers S ...
        if not over and before > cfg[4]:
            assert model[0] == before                           # ... so a scale above max_scale stays where it is on clean steps
    assert state.guards_ok()
    growth, backoff, interval, lo, hi = cfg
    if name in ("floor_holds", "trainstep_ce"):
        assert model[0] == lo
    elif name == "ceiling_holds":
        assert model[0] == hi and seen == {"same"}
    elif name == "above_ceiling":
        assert "down" in seen
    elif name != "interval2000":
        assert {"up", "down", "same"} <= seen                             # the sequence exercised both branches


def test_loss_scale_update_refuses_bad_arguments():
    state = Buf(np.array([64.0, 1.0, 3.0, 2.0], np.float32), F32)
    was = state.raw.clone()
    st = L.stream_ptr()
    for a in ((state.ptr, 0.5, 0.5, 3, 1.0, H32), (state.ptr, 2.0, 0.0, 3, 1.0, H32), (state.ptr, 2.0, -0.1, 3, 1.0, H32),
              (state.ptr, 2.0, 1.5, 3, 1.0, H32), (state.ptr, 2.0, 0.5, 0, 1.0, H32), (state.ptr, 2.0, 0.5, -4, 1.0, H32),
              (None, 2.0, 0.5, 3, 1.0, H32)):
        with pytest.raises(L.SznError):
            L.call("szn_loss_scale_update", *a, st)
    torch.cuda.synchronize()
    assert torch.equal(state.raw, was)


# ---- 5. szn_cast -----------------------------------------------------------------------------------------------------------------------
def _from_bits(patterns):
    return torch.from_numpy(np.array(patterns, np.uint32).view(np.float32).copy())


def all_patterns(dt):
    return torch.from_numpy(np.arange(65536, dtype=np.uint16).view(np.int16).copy()).view(dt)


@functools.lru_cache(maxsize=2)
def cast_inputs(dt):
    """float32 inputs built from the 16-bit grid of `dt`: every representable value, every midpoint between neighbours (an exact tie),
    each midpoint +- one float32 ulp, the overflow threshold, the target's denormals and the tie below the smallest, float32
    denormals, +-0, +-inf, NaNs"""
    grid = all_patterns(dt).float()
    fin = torch.unique(grid[torch.isfinite(grid)].double())                    # sorted
    mid = ((fin[:-1] + fin[1:]) / 2).float()
    assert torch.equal(mid.double(), (fin[:-1] + fin[1:]) / 2)                 # the midpoints are float32 values
    up, dn = torch.nextafter(mid, torch.full_like(mid, INF)), torch.nextafter(mid, torch.full_like(mid, -INF))
    if dt == F16:
        edge = [65504.0, 65519.99, 65520.0, 65520.01, 65536.0, 1e5, 2.0 ** -24, 2.0 ** -25, 2.0 ** -26, 2.0 ** -14, 3 * 2.0 ** -25]
        edge = torch.tensor(edge + [-e for e in edge], dtype=torch.float32)
        edge = torch.cat([edge, torch.nextafter(edge, torch.full_like(edge, INF)), torch.nextafter(edge, torch.full_like(edge, -INF))])
    else:                           # bf16: the largest finite value, the tie above it, +- one ulp, FLT_MAX
        edge = _from_bits([0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7F8001, 0x7F7FFFFF, 0xFF7F0000, 0xFF7F7FFF, 0xFF7F8000, 0xFF7F8001, 0xFF7FFFFF])
    rng = np.random.default_rng(16)
    den = [1, 2, 3, 0x7FFF, 0x8000, 0x8001, 0xFFFF, 0x10000, 0x17FFF, 0x18000, 0x18001, 0x3FFFFF, 0x400000, 0x7FFFFF, 0x800000]
    den += [int(v) for v in rng.integers(1, 0x800000, 2000)]
    den = _from_bits(den + [v | 0x80000000 for v in den])
    spec = _from_bits([0, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FBFFFFF, 0x7FFFFFFF, 0xFF800001])
    allv = torch.cat([grid, mid, up, dn, edge, den, spec])
    return allv[torch.from_numpy(np.random.default_rng(5).permutation(allv.numel()))].contiguous()


def input_class(x):
    """which class of float32 inputs an element belongs to (for the report of a mismatch)"""
    a = np.abs(x)
    return np.where(np.isnan(x), "nan", np.where(np.isinf(x), "inf", np.where((a > 0) & (a < 2.0 ** -126), "f32-denormal", "finite")))


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("n", [1, 255, 257, 2 ** 20 + 1])
def test_cast_f32_to_16bit_is_round_to_nearest_even_on_ties_overflow_and_denormals(dt, n):
    src = cast_inputs(dt)
    # (the large size holds every input at least once; the small ones are windows of the shuffled list)
    src = src.repeat((n + src.numel() - 1) // src.numel())[:n] if n > src.numel() else src[1000 + n:1000 + 2 * n]
    assert src.numel() == n
    want = src.to(dt)
    S, D = Buf(src, F32), Buf(None, dt, n=n)
    L.call("szn_cast", L.SZN_F32, L.dtype_code(dt), n, S.ptr, D.ptr, L.stream_ptr())
    assert L.last_kernel() == "cast_kernel"
    torch.cuda.synchronize()
    assert S.guards_ok() and D.guards_ok() and np.array_equal(S.bits(), fbits(src.numpy()))
    got = D.t.cpu()
    wnan = torch.isnan(want.float())
    assert torch.equal(torch.isnan(got.float()), wnan)                         # NaN -> NaN (any payload), nothing else -> NaN
    bad = ((got.view(torch.int16) != want.view(torch.int16)) & ~wnan).numpy()
    cls = input_class(src.numpy())
    assert not bad.any(), {c: int((bad & (cls == c)).sum()) for c in np.unique(cls[bad])}


@pytest.mark.parametrize("dt", [BF16, F16])
def test_cast_16bit_to_f32_over_all_65536_patterns(dt):
    src = all_patterns(dt)
    want = src.float()
    for n in (65536, 255, 1):
        S, D = Buf(src[:n], dt), Buf(None, F32, n=n)
        L.call("szn_cast", L.dtype_code(dt), L.SZN_F32, n, S.ptr, D.ptr, L.stream_ptr())
        assert L.last_kernel() == "cast_kernel"
        torch.cuda.synchronize()
        assert S.guards_ok() and D.guards_ok()
        got, w = D.t.cpu(), want[:n]
        wnan = torch.isnan(w)
        assert torch.equal(torch.isnan(got), wnan)
        assert torch.equal(got.view(torch.int32)[~wnan], w.view(torch.int32)[~wnan])


@pytest.mark.parametrize("n", [1, 255, 257, 2 ** 20 + 1])
def test_cast_f32_to_f32_copies_bits_and_bad_calls_are_refused(n):
    src = cast_inputs(BF16)
    src = src.repeat((n + src.numel() - 1) // src.numel())[:n]
    S, D = Buf(src, F32), Buf(None, F32, n=n)
    st = L.stream_ptr()
    L.call("szn_cast", L.SZN_F32, L.SZN_F32, n, S.ptr, D.ptr, st)
    assert L.last_kernel() == "cast_kernel"
    torch.cuda.synchronize()
    assert D.guards_ok() and np.array_equal(D.bits(), fbits(src.numpy()))     # NaN payloads and denormals included
    E = Buf(None, F32, n=n)
    L.call("szn_cast", L.SZN_F32, L.SZN_F32, 0, S.ptr, E.ptr, st)             # n = 0: OK, nothing written
    for a in ((L.SZN_BF16, L.SZN_F16, n, S.ptr, E.ptr), (L.SZN_BF16, L.SZN_BF16, n, S.ptr, E.ptr), (L.SZN_F32, 5, n, S.ptr, E.ptr),
              (-1, L.SZN_F32, n, S.ptr, E.ptr), (L.SZN_F32, L.SZN_F32, -1, S.ptr, E.ptr), (L.SZN_F32, L.SZN_F32, n, None, E.ptr),
              (L.SZN_F32, L.SZN_F32, n, S.ptr, None)):
        with pytest.raises(L.SznError):
            L.call("szn_cast", *a, st)
    torch.cuda.synchronize()
    assert bool((E.raw == SENT[4]).all())


# ---- 6. szn_dropout2d_mask ---------------------------------------------------------------------------------------------------------------
SEEDS = (0, 1337, 1337 + 7919, 2 ** 63 + 5)
OFFSETS = (0, 1 << 24, 5 << 24, 2 ** 40)


def gpu_mask(n, p, seed, offset):
    B = Buf(None, F32, n=n)
    L.call("szn_dropout2d_mask", n, p, seed, offset, B.ptr, L.stream_ptr())
    assert L.last_kernel() == "dropout_mask_kernel"
    torch.cuda.synchronize()
    assert B.guards_ok()                                        # the buffer beyond n is untouched
    return B.np()


@pytest.mark.parametrize("p", [0.0, 0.25, 0.5, 0.9])
@pytest.mark.parametrize("n", [1, 255, 32768, 100003])
def test_dropout_mask_is_the_reference_generator_bit_for_bit(p, n):
    keep = np.float32(1) / (np.float32(1) - np.float32(p))
    for seed, offset in itertools.product(SEEDS, OFFSETS):
        got = gpu_mask(n, p, seed, offset)
        assert np.array_equal(fbits(got), fbits(H.dropout_ref(n, p, seed, offset))), (p, n, seed, offset)
        assert np.all((got == 0) | (got == keep))
        if p == 0.0:
            assert np.all(got == 1.0)


def test_dropout_offset_contract_rank_seeds_and_refusals():
    n = 4096
    for seed, offset in ((1337, 0), (1337 + 7919, 3 << 24), (2 ** 63 + 5, 2 ** 40)):
        base = gpu_mask(n + 1000, 0.5, seed, offset)
        for k in (1, 255, 256, 1000):                           # mask(seed, offset + k)[i] == mask(seed, offset)[i + k]
            assert np.array_equal(gpu_mask(n, 0.5, seed, offset + k), base[k:k + n])
    # the seeds of data-parallel ranks 0 and 1, and consecutive calls of one rank (offset k << 24), draw different masks
    a = [gpu_mask(32768, 0.5, 1337 + 7919 * r, k << 24) != 0 for r in (0, 1) for k in (0, 1)]
    sigma = np.sqrt(0.25 / 32768)
    for i, j in itertools.combinations(range(4), 2):
        assert abs(float((a[i] == a[j]).mean()) - 0.5) <= 5 * sigma
    B = Buf(None, F32, n=64)
    for bad in ((64, -0.1, 1, 0, B.ptr), (64, 1.0, 1, 0, B.ptr), (64, 1.5, 1, 0, B.ptr), (0, 0.5, 1, 0, B.ptr), (-3, 0.5, 1, 0, B.ptr),
                (64, 0.5, 1, 0, None)):
        with pytest.raises(L.SznError):
            L.call("szn_dropout2d_mask", *bad, L.stream_ptr())
    torch.cuda.synchronize()
    assert bool((B.raw == SENT[4]).all())
