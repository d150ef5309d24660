"""GPU: precision bf16x3 (SZN_BF16X3) -- fp32 tensors, conv GEMMs on the bf16 matrix cores with every operand split into hi + lo.

Per kernel: forward / dgrad / wgrad on shapes that reach every fp32 dispatch route, against an fp64 referee on the CPU (relative L2
<= 4e-5; the error model of include/szn.h predicts a few e-6, plain bf16 operands give ~3e-3).  Then one full training step against the
CPU oracle and short training runs against the fp32 path."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import szn_oracle as O  # noqa: E402
from helpers_parity import adopt_forward  # noqa: E402
from zeroshotsemanticsegmentation_amd import _lib as L  # noqa: E402
from zeroshotsemanticsegmentation_amd import engine, models, synth  # noqa: E402

X3 = L.SZN_BF16X3


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def rel_l2(got, ref):
    got, ref = got.double(), ref.double()
    return float((got - ref).norm() / ref.norm())


def x3_kernel():
    """the split kernel the last call ran (the GEMM may sit in front of a split-K / slab / col2im pass)"""
    for k in (L.last_kernel(), L.prev_kernel()):
        if k.endswith("+bf16x3"):
            return k
    return None


# B, Hi, Wi, Ci, Co, K, pad -> the split kernel the forward, dgrad and wgrad must report (a|b: the split-K cost model picks the tiling)
CASES = {
    (2, 19, 23, 64, 96, 3, 1): ("conv_igemm_v2", "conv_igemm_v2", "conv_wgrad_v2"),       # 256 x 128 tiles; dgrad: 64-wide tile
    (1, 33, 47, 64, 64, 3, 1): ("conv_igemm_v2", "conv_igemm_v2", "conv_wgrad_v2"),       # 256 x 64 tiles, odd map, B = 1
    (2, 128, 128, 64, 512, 1, 0): ("conv_igemm_wide", "conv_igemm_v2", "conv_wgrad_v2"),  # 256 x 256 tiles (conv_igemm_wide<., 8>)
    (2, 8, 8, 512, 128, 7, 0): ("conv_igemm_v2", "conv_igemm_v2|conv_igemm_wide", "conv_wgrad_v2"),   # few tiles, long K: split-K
    (2, 7, 7, 1024, 1024, 1, 0): ("conv_igemm_v2", "conv_igemm_v2", "conv_wgrad_v2"),     # fc7-like 1x1
    (1, 1, 33000, 32, 64, 1, 0): ("conv_igemm", "conv_igemm", "conv_wgrad_v2"),           # >= 32000 columns: first-generation kernel
}


def _run(fn):
    fn()
    k = x3_kernel()
    torch.cuda.synchronize()
    return k


@pytest.mark.parametrize("case", list(CASES))
def test_split_conv_kernels_vs_fp64(case):
    B, Hi, Wi, Ci, Co, K, pad = case
    g = torch.Generator().manual_seed(4242 + Ci + Co + Wi)
    x = torch.randn(B, Ci, Hi, Wi, generator=g, dtype=torch.float64)
    w = torch.randn(Co, Ci, K, K, generator=g, dtype=torch.float64) / (Ci * K * K) ** 0.5
    bias = torch.randn(Co, generator=g, dtype=torch.float64)
    x, w = x.float().double(), w.float().double()              # the operands the kernels see (fp32)
    Ho, Wo = Hi + 2 * pad - K + 1, Wi + 2 * pad - K + 1
    dout = torch.randn(B, Co, Ho, Wo, generator=g, dtype=torch.float64).float().double()
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    yr = F.conv2d(xr, wr, bias, padding=pad)
    yr.backward(dout)
    dev = "cuda"
    xd, wd, bd = nhwc(x).float().to(dev), nhwc(w).float().to(dev), bias.float().to(dev)
    dd = nhwc(dout).float().to(dev)
    ws = torch.empty(max(B * Ho * Wo * Co, B * Hi * Wi * Ci) * 4 * 16, dtype=torch.uint8, device=dev)
    wT = torch.empty(Ci, K, K, Co, device=dev)
    L.call("szn_pack_weight_dgrad", X3, Co, K, K, Ci, L.ptr(wd), L.ptr(wT), L.stream_ptr())

    def desc(dt):
        d = L.ConvDesc(dt, B, Hi, Wi, Ci, Ho, Wo, Co, K, K, pad, Ci, Co, 0, 0, 0)
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
        return d

    def fwd(dt, xs=xd, wsrc=wd):
        out = torch.full((B, Ho, Wo, Co), float("nan"), device=dev)
        k = _run(lambda: L.call("szn_conv2d_fwd", C.byref(desc(dt)), L.ptr(xs), L.ptr(wsrc), L.ptr(bd), None, None, L.ptr(out),
                                L.stream_ptr()))
        return out, k

    def dgrad(dt, wTs=wT):
        din = torch.full((B, Hi, Wi, Ci), float("nan"), device=dev)
        k = _run(lambda: L.call("szn_conv2d_dgrad", C.byref(desc(dt)), L.ptr(dd), L.ptr(wTs), None, None, L.ptr(din), L.stream_ptr()))
        return din, k

    def wgrad(dt, xs=xd, ds=dd):
        dw = torch.full((Co, K, K, Ci), float("nan"), device=dev)
        k = _run(lambda: L.call("szn_conv2d_wgrad", C.byref(desc(dt)), L.ptr(xs), L.ptr(ds), L.ptr(dw), 0, L.stream_ptr()))
        return dw, k

    refs = {"fwd": nhwc(yr.detach()), "dgrad": nhwc(xr.grad), "wgrad": nhwc(wr.grad)}
    runs = {"fwd": fwd, "dgrad": dgrad, "wgrad": wgrad}
    for i, what in enumerate(("fwd", "dgrad", "wgrad")):
        got, kern = runs[what](X3)
        again, _ = runs[what](X3)
        f32, _ = runs[what](L.SZN_F32)
        e_x3, e_f32 = rel_l2(got.cpu(), refs[what]), rel_l2(f32.cpu(), refs[what])
        # plain bf16 operands on the same inputs, for the record (16-bit tensors need Ci / Co multiples of 64 on these paths)
        e_bf = float("nan")
        if Ci % 64 == 0 and Co % 64 == 0:
            bt = torch.bfloat16
            out_b = {"fwd": torch.empty(B, Ho, Wo, Co, device=dev, dtype=bt), "dgrad": torch.empty(B, Hi, Wi, Ci, device=dev, dtype=bt),
                     "wgrad": torch.empty(Co, K, K, Ci, device=dev)}[what]
            a1, a2 = {"fwd": (xd, wd), "dgrad": (dd, wT), "wgrad": (xd, dd)}[what]
            a1, a2 = a1.to(bt), a2.to(bt)
            if what == "fwd":
                L.call("szn_conv2d_fwd", C.byref(desc(L.SZN_BF16)), L.ptr(a1), L.ptr(a2), L.ptr(bd), None, None, L.ptr(out_b), L.stream_ptr())
            elif what == "dgrad":
                L.call("szn_conv2d_dgrad", C.byref(desc(L.SZN_BF16)), L.ptr(a1), L.ptr(a2), None, None, L.ptr(out_b), L.stream_ptr())
            else:
                L.call("szn_conv2d_wgrad", C.byref(desc(L.SZN_BF16)), L.ptr(a1), L.ptr(a2), L.ptr(out_b), 0, L.stream_ptr())
            torch.cuda.synchronize()
            e_bf = rel_l2(out_b.float().cpu(), refs[what])
        print("%s %-6s bf16x3 %.2e  fp32 %.2e  bf16 %.2e  (%s)" % (case, what, e_x3, e_f32, e_bf, kern))
        assert kern in [k + "+bf16x3" for k in CASES[case][i].split("|")], (what, L.prev_kernel(), L.last_kernel())
        assert e_x3 <= 4e-5, (what, e_x3)
        assert torch.equal(got, again), what                   # deterministic
        assert not torch.equal(got, f32), what                 # it really is a different arithmetic


def test_fc6_dgrad_gemm_col2im():
    """fc6's backward-data as GEMM + col2im (szn_conv2d_dgrad_gemm): the GEMM in front of col2im is the split kernel"""
    B, Hi, Wi, Ci, Co, K = 2, 23, 23, 512, 256, 7
    g = torch.Generator().manual_seed(606)
    w = (torch.randn(Co, Ci, K, K, generator=g, dtype=torch.float64) / (Ci * K * K) ** 0.5).float().double()
    Ho, Wo = Hi - K + 1, Wi - K + 1
    dout = torch.randn(B, Co, Ho, Wo, generator=g, dtype=torch.float64).float().double()
    ref = nhwc(torch.nn.grad.conv2d_input((B, Ci, Hi, Wi), w, dout))
    dev = "cuda"
    wd = nhwc(w).float().to(dev)
    wG = torch.empty(K * K * Ci, Co, device=dev)
    L.call("szn_pack_weight_dgrad", X3, Co, 1, 1, K * K * Ci, L.ptr(wd), L.ptr(wG), L.stream_ptr())
    d = L.ConvDesc(X3, B, Hi, Wi, Ci, Ho, Wo, Co, K, K, 0, Ci, Co, 0, 0, 0)
    lib = L.load()
    assert lib.szn_conv2d_dgrad_gemm_native_supported(C.byref(d)) == 0          # as for SZN_F32: the 16-bit native form only
    nb = lib.szn_conv2d_dgrad_gemm_workspace_bytes(C.byref(d))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    d.workspace, d.workspace_bytes = ws.data_ptr(), nb
    dd = nhwc(dout).float().to(dev)

    def run(dt):
        d.dtype = dt
        din = torch.full((B, Hi, Wi, Ci), float("nan"), device=dev)
        L.call("szn_conv2d_dgrad_gemm", C.byref(d), L.ptr(dd), L.ptr(wG), L.ptr(din), L.stream_ptr())
        kern = (L.prev_kernel(), L.last_kernel())
        torch.cuda.synchronize()
        return din, kern

    got, kern = run(X3)
    again, _ = run(X3)
    f32, _ = run(L.SZN_F32)
    e = rel_l2(got.cpu(), ref)
    print("fc6 dgrad GEMM + col2im: bf16x3 %.2e  fp32 %.2e  %s" % (e, rel_l2(f32.cpu(), ref), kern))
    assert kern[1] == "col2im_kernel" and kern[0].endswith("+bf16x3"), kern
    assert e <= 4e-5
    assert torch.equal(got, again) and not torch.equal(got, f32)


def test_non_gemm_entry_points_reject_bf16x3():
    dev = "cuda"
    x = torch.zeros(1, 4, 4, 64, device=dev)
    y = torch.zeros(1, 2, 2, 64, device=dev)
    L.call("szn_maxpool2x2_ceil_fwd", L.SZN_F32, 1, 4, 4, 64, L.ptr(x), L.ptr(y), L.stream_ptr())
    assert L.last_kernel() == "maxpool_fwd_kernel"
    L.call("szn_cast", L.SZN_F32, L.SZN_F32, 16, L.ptr(x), L.ptr(y), L.stream_ptr())
    before = L.last_kernel()
    db = torch.zeros(64, device=dev)
    for name, args in (("szn_maxpool2x2_ceil_fwd", (X3, 1, 4, 4, 64, L.ptr(x), L.ptr(y), L.stream_ptr())),
                       ("szn_cast", (X3, L.SZN_F32, 16, L.ptr(x), L.ptr(y), L.stream_ptr())),
                       ("szn_cast", (L.SZN_F32, X3, 16, L.ptr(x), L.ptr(y), L.stream_ptr())),
                       ("szn_bias_grad", (X3, 16, 64, 64, L.ptr(x), L.ptr(db), 0, L.stream_ptr()))):
        with pytest.raises(L.SznError) as ei:
            L.call(name, *args)
        assert "bad" in str(ei.value) or "unsupported" in str(ei.value), (name, str(ei.value))
        assert L.last_kernel() == before, (name, L.last_kernel())        # nothing launched
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- one full step vs the oracle
def _grad_errors(m, og, keys):
    out = {}
    for key in keys:
        name, kind = key.split(".")
        gg = getattr(getattr(m, name), kind).grad.detach().cpu().numpy().astype(np.float64)
        r = og[key].astype(np.float64)
        out[key] = float(np.abs(gg - r).max() / np.abs(r).max())
    return out


def _margins(f, emb):
    E = f.shape[1]
    sc = f[0].reshape(E, -1).T.astype(np.float64)
    en = np.linalg.norm(emb.astype(np.float64), axis=1)
    en[en == 0] = 1.0
    sim = sc @ emb.astype(np.float64).T / (np.linalg.norm(sc, axis=1, keepdims=True) * en[None, :])
    top2 = np.sort(sim, axis=1)[:, -2:]
    return (top2[:, 1] - top2[:, 0]).reshape(f.shape[2:])


def test_train_step_vs_oracle():
    """one TrainStep(precision='bf16x3') step, E = 300, K = 59, Dropout2d on: loss and class map against the oracle's forward,
    every gradient against the oracle's backward on the step's own forward state (tests/helpers_parity.py)"""
    E, K, H = 300, 59, 256
    emb = synth.make_embeddings(K, E)
    x = synth.make_images(1, H, H, seed=31)
    target = synth.make_labels(1, H, H, K, seed=32, classes=list(range(49)))
    m = models.FCN32s(E)
    m.load_synthetic(1337, device=torch.device("cuda"))
    params = {k: v.detach().cpu().numpy() for k, v in m.named_parameters() if k.split(".")[0] != "upscore"}
    m.train()
    eng = m._engine
    calls = eng.dropout_calls
    masks = [t.cpu().numpy() for t in eng.make_masks(1, 4096, torch.device("cuda"))]
    eng.dropout_calls = calls                                  # the step draws exactly these
    of = O.FCN32sOracle(params, E).forward(x, "fcn", masks=masks)
    ts = engine.TrainStep(m, emb, optimizer="adam", lr=1e-5, precision="bf16x3", fused_head=True)
    ts.keep_ctx = True
    try:
        loss, pred = ts.step(torch.from_numpy(x).cuda(), torch.from_numpy(target).cuda())
        torch.cuda.synchronize()
        oloss, _, _ = O.cosine_loss(of, target, embed=emb)
        print("loss bf16x3 %.7f  oracle %.7f" % (loss.item(), float(oloss)))
        assert abs(loss.item() - float(oloss)) < 1e-4 * max(1.0, abs(float(oloss)))
        clear = _margins(of, emb)[None] > 1e-4
        assert np.array_equal(pred.cpu().numpy()[clear], O.infer_lbl(of, emb)[clear])
        om = O.FCN32sOracle(params, E)
        adopt_forward(om, ts.last_ctx, x, masks, E)
        f_hip = O.deconv_fwd(om.saved["coarse_f"], np.broadcast_to(O.get_upsampling_weight(1, 1, 64)[0, 0], (E, 64, 64)), H, H, diag=True)
        _, odf, _ = O.cosine_loss(f_hip, target, embed=emb)
        og = om.backward(df=odf)
        keys = ["%s.%s" % (n, k) for n in models._OPT_LAYERS for k in ("weight", "bias")]
        errs = _grad_errors(m, og, keys)
        print("gradient errors given the same forward state (max over the tensor / max |ref|):")
        for k in keys:
            print("  %-16s %.2e" % (k, errs[k]))
        for k, e in errs.items():
            assert e < 1e-3, (k, e)
    finally:
        ts.last_ctx = None


# ------------------------------------------------------------------------------------------------- against the fp32 path
def _train(precision, steps):
    E, K, H, W, B = 20, 18, 64, 64, 2
    emb = synth.make_embeddings(K, E)
    x = torch.from_numpy(synth.make_images(B, H, W, seed=5)).cuda()
    t = torch.from_numpy(synth.make_labels(B, H, W, K, seed=6, block=8)).cuda()
    m = models.FCN32s(E)
    m.load_synthetic(1337, device=torch.device("cuda"))
    m.eval()
    ts = engine.TrainStep(m, emb, optimizer="adam", lr=1e-4, precision=precision, fused_head=True)
    losses = [float(ts.step(x, t)[0]) for _ in range(steps)]
    torch.cuda.synchronize()
    return losses


def test_training_follows_fp32():
    a, b = _train(torch.float32, 30), _train("bf16x3", 30)
    print("fp32   %.6f -> %.6f\nbf16x3 %.6f -> %.6f" % (a[0], a[-1], b[0], b[-1]))
    assert abs(a[0] - b[0]) < 1e-4
    assert b[-1] < b[0] - 0.5 * (a[0] - a[-1])                 # it learns as fp32 does
    assert abs(a[-1] - b[-1]) < 0.1 * (a[0] - a[-1]) + 1e-3


def test_train_cli_synthetic():
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "-c", "18", "-g", "0", "--synthetic", "2", "64", "64",
                            "--precision", "bf16x3", "-dir", d, "--workers", "0"], cwd=ROOT, timeout=300,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-3000:]
