"""GPU parity tests of the MFMA convolution kernels (forward / dgrad / wgrad, conv1_1, pools) through the
C-ABI, against a plain torch fp32 reference of the same op computed on the CPU (floating-point kernels).

Tolerances: fp32 path 1e-3 relative (north_star), measured ~1e-6; bf16 path compares against the fp32
reference evaluated on bf16-rounded operands with 2e-2 relative to the output scale.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from zeroshotsemanticsegmentation_amd import _lib as L


def nhwc(t):  # (B,C,H,W) logical -> physical NHWC contiguous tensor [B][H][W][C]
    return t.permute(0, 2, 3, 1).contiguous()


def relerr(a, b):
    a, b = a.double(), b.double()
    a, b = a.detach(), b.detach()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


CASES = [
    # B, Hi, Wi, Ci, Co, K, pad
    (2, 19, 23, 64, 96, 3, 1),
    (1, 9, 9, 128, 200, 7, 0),
    (3, 5, 7, 192, 302, 1, 0),
    (1, 33, 17, 64, 64, 3, 1),
    (2, 12, 12, 64, 130, 3, 2),
    (1, 40, 36, 256, 64, 3, 1),          # 64-cout tile variant, several pixel tiles, 4 chunks per tap
    (2, 8, 8, 512, 128, 7, 0),           # long K (392 chunks bf16), 1 pixel tile: split-K path
    (1, 20, 21, 64, 256, 3, 1),          # 256-cout tiles (szn_conv_wide.hip when SZN_WIDE_MINTILES allows), 2 pixel tiles
    (2, 10, 9, 128, 512, 1, 0),          # 2 cout tiles of 256
    (1, 9, 9, 256, 512, 7, 0),           # wgrad: 256 x 256 tiles (szn_conv_wgrad_wide.hip), 98 tiles, one K step
    (2, 7, 6, 448, 512, 5, 1),           # wgrad wide with a ragged cin tile (448 = 256 + 192) and padding taps
    (1, 260, 260, 64, 300, 1, 0),        # the 300-d projection shape: one 320-wide cout tile (bf16), >= 256 pixel tiles
    (2, 260, 250, 64, 64, 3, 1),         # register-resident filter bank (szn_conv_regw.hip, bf16), ragged edges; wgrad_taps
    (1, 181, 190, 64, 128, 3, 1),        # regw <COG 4, CIG 1>: 8-row tiles
    (1, 190, 181, 128, 64, 3, 1),        # regw <2, 2>: cin halves in partner waves, exchange through LDS
    (1, 183, 187, 128, 128, 3, 1),       # regw <4, 2>: 4-row tiles
    (3, 150, 151, 64, 256, 3, 1),        # row-resident 3x3 wide kernel (bf16): one cin chunk, tiles run across rows and images
    (1, 260, 258, 256, 256, 3, 1),       # ... four cin chunks, forward and dgrad, ragged last tile
    (37, 43, 42, 64, 256, 3, 1),         # ... small maps: every 256-pixel tile crosses image boundaries
    (1, 3, 25000, 64, 256, 3, 1),        # ... three very long rows: two thirds of the pixels are border pixels in the vertical direction
    (5, 32, 32, 64, 2000, 1, 0),         # 256 x 192 tiles (bf16): 20 x 11 = 220 tiles in one round where 256 x 128 needs 320; ragged last tile
    (8, 17, 17, 4096, 4096, 1, 0),       # ... fc7 at the bench shape, forward and dgrad (gate, column sums)
]


# which kernel the dispatcher must pick in bf16 (forward, dgrad, wgrad) for the cases that exist to cover a specialised
# path: a silent fallback to the generic kernel would still be numerically right, so it is asserted by name
EXPECT_BF16 = {
    (2, 260, 250, 64, 64, 3, 1): ("conv3x3_regw", "conv3x3_regw", "wgrad_taps_reduce"),
    (1, 181, 190, 64, 128, 3, 1): ("conv3x3_regw", "conv3x3_regw", "wgrad_taps_reduce"),
    (1, 190, 181, 128, 64, 3, 1): ("conv3x3_regw", "conv3x3_regw", "wgrad_taps_reduce"),
    (1, 183, 187, 128, 128, 3, 1): ("conv3x3_regw", "conv3x3_regw", "wgrad_taps_reduce"),
    (1, 260, 260, 64, 300, 1, 0): ("conv_igemm_wide", None, None),
    (5, 32, 32, 64, 2000, 1, 0): ("conv_igemm_wide", None, None),
    (8, 17, 17, 4096, 4096, 1, 0): ("conv_igemm_wide", "conv_igemm_wide", "conv_wgrad_wide"),
    (3, 150, 151, 64, 256, 3, 1): ("conv_igemm_8ph", None, None),
    (1, 260, 258, 256, 256, 3, 1): ("conv_igemm_8ph", "conv_igemm_8ph", None),
    (37, 43, 42, 64, 256, 3, 1): ("conv_igemm_8ph", None, None),
    (1, 3, 25000, 64, 256, 3, 1): ("conv_igemm_8ph", None, None),
    (1, 9, 9, 256, 512, 7, 0): (None, None, "conv_wgrad_wide"),
    (2, 7, 6, 448, 512, 5, 1): (None, None, "conv_wgrad_wide"),
    (2, 8, 8, 512, 128, 7, 0): ("splitk_epilogue", None, None),
}


def conv_desc(dt, B, Hi, Wi, Ci, Co, K, pad, relu=0, out_f32=0, ldg=0):
    Ho, Wo = Hi + 2 * pad - K + 1, Wi + 2 * pad - K + 1
    ldo = (Co + 7) // 8 * 8          # padded pixel stride of the output (e.g. 302 -> 304)
    return L.ConvDesc(dt, B, Hi, Wi, Ci, Ho, Wo, Co, K, K, pad, Ci, ldo, ldg, relu, out_f32), Ho, Wo


def pad_c(t, ld):  # NHWC tensor -> channel dimension zero-padded to ld
    return F.pad(t, (0, ld - t.shape[-1])).contiguous()


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_conv_fwd_dgrad_wgrad(case, dtype):
    B, Hi, Wi, Ci, Co, K, pad = case
    g = torch.Generator().manual_seed(1337 + Ci + Co)
    x = torch.randn(B, Ci, Hi, Wi, generator=g)
    w = torch.randn(Co, Ci, K, K, generator=g) / (Ci * K * K) ** 0.5
    bias = torch.randn(Co, generator=g)
    if dtype == torch.bfloat16:
        x, w = x.bfloat16().float(), w.bfloat16().float()
    x.requires_grad_(True); w.requires_grad_(True)
    ref = F.relu(F.conv2d(x, w, bias, padding=pad))
    dt = L.dtype_code(dtype)
    d, Ho, Wo = conv_desc(dt, B, Hi, Wi, Ci, Co, K, pad, relu=1)
    dev = "cuda"
    # split-K scratch (used by the library only for few-tile / long-K shapes such as case 1)
    ws = torch.empty(max(B * Ho * Wo * Co, B * Hi * Wi * Ci) * 4, dtype=torch.uint8, device=dev)
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    xd = nhwc(x.detach()).to(dev, dtype)
    wd = nhwc(w.detach()).to(dev, dtype)       # OHWI
    bd = bias.to(dev)
    out = torch.full((B, Ho, Wo, d.ldo), float("nan"), device=dev, dtype=dtype)
    L.call("szn_conv2d_fwd", C.byref(d), L.ptr(xd), L.ptr(wd), L.ptr(bd), None, None, L.ptr(out), L.stream_ptr())
    expect = EXPECT_BF16.get(case, (None, None, None)) if dtype == torch.bfloat16 else (None, None, None)
    if expect[0]:
        assert L.last_kernel() == expect[0], ("fwd kernel", L.last_kernel())
    torch.cuda.synchronize()
    got = out[..., :Co].float().cpu().permute(0, 3, 1, 2)
    tol = 1e-5 if dtype == torch.float32 else 1e-2
    assert relerr(got, ref) < tol, ("fwd", relerr(got, ref))

    # ---- fused MaxPool2d(2,2,ceil) of the output (descriptor.pool_out): exactly the pool of the stored tensor
    if d.ldo == Co:
        pooled = torch.full((B, (Ho + 1) // 2, (Wo + 1) // 2, Co), float("nan"), device=dev, dtype=dtype)
        out2 = torch.full_like(out, float("nan"))
        d.pool_out = pooled.data_ptr()
        L.call("szn_conv2d_fwd", C.byref(d), L.ptr(xd), L.ptr(wd), L.ptr(bd), None, None, L.ptr(out2), L.stream_ptr())
        if expect[0] == "conv3x3_regw":
            assert L.last_kernel() == "conv3x3_regw", L.last_kernel()      # pooled inside the conv epilogue
        else:
            assert L.last_kernel() == "maxpool_fwd_kernel", L.last_kernel()
        d.pool_out = None
        torch.cuda.synchronize()
        assert torch.equal(out2, out)
        pref = F.max_pool2d(out.float().permute(0, 3, 1, 2), 2, 2, ceil_mode=True).permute(0, 2, 3, 1)
        assert torch.equal(pooled.float(), pref)

    # ---- backward: dout random, gate = x > 0 is applied by the dgrad epilogue
    dout = torch.randn(B, Co, Ho, Wo, generator=g)
    if dtype == torch.bfloat16:
        dout = dout.bfloat16().float()
    pre = F.conv2d(x, w, bias, padding=pad)
    pre.backward(dout)
    dx_ref = x.grad * (x.detach() > 0)
    dw_ref = w.grad
    db_ref = dout.sum((0, 2, 3))
    doutd = pad_c(nhwc(dout), d.ldo).to(dev, dtype)
    wT = torch.empty(Ci, K, K, Co, device=dev, dtype=dtype)
    L.call("szn_pack_weight_dgrad", dt, Co, K, K, Ci, L.ptr(wd), L.ptr(wT), L.stream_ptr())
    wT_ref = w.detach().flip(2, 3).permute(1, 2, 3, 0).contiguous()
    torch.cuda.synchronize()
    assert torch.equal(wT.float().cpu(), wT_ref.to(dtype).float())
    dgd, _, _ = conv_desc(dt, B, Hi, Wi, Ci, Co, K, pad, ldg=Ci)
    dgd.workspace, dgd.workspace_bytes = ws.data_ptr(), ws.numel()
    din = torch.full((B, Hi, Wi, Ci), float("nan"), device=dev, dtype=dtype)
    if Co % (64 if dtype == torch.bfloat16 else 32) == 0:
        L.call("szn_conv2d_dgrad", C.byref(dgd), L.ptr(doutd), L.ptr(wT), L.ptr(xd), None, L.ptr(din), L.stream_ptr())
        if expect[1]:
            assert L.last_kernel() == expect[1], ("dgrad kernel", L.last_kernel())
        torch.cuda.synchronize()
        got = din.float().cpu().permute(0, 3, 1, 2)
        assert relerr(got, dx_ref) < tol, ("dgrad", relerr(got, dx_ref))
        # fused column sums (bias gradient of the producer layer); split-K is off on this path
        cs = torch.zeros(Ci, device=dev)
        dgc, _, _ = conv_desc(dt, B, Hi, Wi, Ci, Co, K, pad, ldg=Ci)
        dgc.colsum = cs.data_ptr()
        din2 = torch.empty_like(din)
        L.call("szn_conv2d_dgrad", C.byref(dgc), L.ptr(doutd), L.ptr(wT), L.ptr(xd), None, L.ptr(din2), L.stream_ptr())
        torch.cuda.synchronize()
        assert relerr(din2.float().cpu().permute(0, 3, 1, 2), dx_ref) < tol
        # the sums are taken on the fp32 values before the bf16 rounding of din
        assert relerr(cs.cpu(), dx_ref.sum((0, 2, 3))) < (1e-4 if dtype == torch.float32 else 1e-2)

        # deterministic form: partial rows in a slab (NaN-filled: every row the kernel reports must be written completely) +
        # szn_colsum_reduce_batch; equal to the atomics to rounding, bit-identical from run to run
        def slab_colsum():
            cs2 = torch.zeros(Ci, device=dev)
            cap = max((B * Hi * Wi + 255) // 256, 2048)
            slab = torch.full((cap * Ci,), float("nan"), device=dev)
            dgs, _, _ = conv_desc(dt, B, Hi, Wi, Ci, Co, K, pad, ldg=Ci)
            dgs.colsum, dgs.colsum_slab, dgs.colsum_slab_rows = cs2.data_ptr(), slab.data_ptr(), cap
            L.call("szn_conv2d_dgrad", C.byref(dgs), L.ptr(doutd), L.ptr(wT), L.ptr(xd), None, L.ptr(din2), L.stream_ptr())
            rows = dgs.res.colsum_rows
            assert 0 < rows <= cap
            assert float(cs2.abs().max()) == 0.0                    # the kernel itself leaves colsum alone
            L.call("szn_colsum_reduce_batch", 1, (C.c_void_p * 1)(slab.data_ptr()), (C.c_int * 1)(rows), (C.c_int * 1)(Ci),
                   (C.c_void_p * 1)(cs2.data_ptr()), L.stream_ptr())
            torch.cuda.synchronize()
            return cs2
        ca, cb = slab_colsum(), slab_colsum()
        assert torch.equal(ca, cb)
        assert relerr(ca.cpu(), cs.cpu()) < 1e-5
    dw = torch.full((Co, K, K, Ci), float("nan"), device=dev)
    db = torch.full((Co,), float("nan"), device=dev)
    L.call("szn_conv2d_wgrad", C.byref(dgd), L.ptr(xd), L.ptr(doutd), L.ptr(dw), 0, L.stream_ptr())
    if expect[2]:
        assert L.last_kernel() == expect[2], ("wgrad kernel", L.last_kernel())
    L.call("szn_bias_grad", dt, B * Ho * Wo, Co, d.ldo, L.ptr(doutd), L.ptr(db), 0, L.stream_ptr())
    # ... and its deterministic form
    db2 = torch.full((Co,), float("nan"), device=dev)
    bslab = torch.full((2048 * Co,), float("nan"), device=dev)
    bro = L.rows_out()
    L.call("szn_bias_grad_slab", dt, B * Ho * Wo, Co, d.ldo, L.ptr(doutd), L.ptr(db2), 0, L.ptr(bslab), 2048, C.byref(bro), L.stream_ptr())
    brows = bro.value
    L.call("szn_colsum_reduce_batch", 1, (C.c_void_p * 1)(bslab.data_ptr()), (C.c_int * 1)(brows), (C.c_int * 1)(Co),
           (C.c_void_p * 1)(db2.data_ptr()), L.stream_ptr())
    torch.cuda.synchronize()
    assert 0 < brows <= 2048 and relerr(db2.cpu(), db_ref) < 1e-4
    got = dw.cpu().permute(0, 3, 1, 2)
    # a weight gradient sums B*Ho*Wo products per entry: the fp32 reduction-order noise (vs torch's own order) grows with the
    # pixel count (1.1e-5 at 66 k pixels)
    wtol = tol * (3.0 if (dtype == torch.float32 and B * Ho * Wo > 50000) else 1.0)
    assert relerr(got, dw_ref) < wtol, ("wgrad", relerr(got, dw_ref))
    assert relerr(db.cpu(), db_ref) < 1e-4, ("bias", relerr(db.cpu(), db_ref))
    # accumulate = 1 adds on top
    L.call("szn_conv2d_wgrad", C.byref(dgd), L.ptr(xd), L.ptr(doutd), L.ptr(dw), 1, L.stream_ptr())
    torch.cuda.synchronize()
    assert relerr(dw.cpu().permute(0, 3, 1, 2), 2 * dw_ref) < wtol


@pytest.mark.parametrize("case", [(2, 8, 8, 512, 128, 7, 0), (2, 7, 6, 448, 512, 5, 1), (1, 9, 9, 128, 200, 7, 0),
                                  (2, 23, 23, 512, 256, 7, 0)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_conv_dgrad_gemm_col2im(case, dtype):
    """szn_conv2d_dgrad_gemm (fc6's backward-data as GEMM + col2im) against torch's conv backward"""
    B, Hi, Wi, Ci, Co, K, pad = case
    g = torch.Generator().manual_seed(77 + Ci + Co)
    x = torch.randn(B, Ci, Hi, Wi, generator=g, requires_grad=True)
    w = torch.randn(Co, Ci, K, K, generator=g) / (Ci * K * K) ** 0.5
    if dtype == torch.bfloat16:
        w = w.bfloat16().float()
    out = F.conv2d(x, w, None, padding=pad)
    Ho, Wo = out.shape[2:]
    dout = torch.randn(B, Co, Ho, Wo, generator=g)
    if dtype == torch.bfloat16:
        dout = dout.bfloat16().float()
    out.backward(dout)
    dt = L.dtype_code(dtype)
    dev = "cuda"
    wd = nhwc(w).to(dev, dtype)                                   # OHWI
    wG = torch.empty(K * K * Ci, Co, device=dev, dtype=dtype)
    L.call("szn_pack_weight_dgrad", dt, Co, 1, 1, K * K * Ci, L.ptr(wd), L.ptr(wG), L.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(wG.float().cpu(), nhwc(w).reshape(Co, -1).t().to(dtype).float())
    d, _, _ = conv_desc(dt, B, Hi, Wi, Ci, Co, K, pad)
    nb = L.load().szn_conv2d_dgrad_gemm_workspace_bytes(C.byref(d))
    assert nb == B * Ho * Wo * K * K * Ci * 4
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    d.workspace, d.workspace_bytes = ws.data_ptr(), nb
    doutd = pad_c(nhwc(dout), d.ldo).to(dev, dtype)
    din = torch.full((B, Hi, Wi, Ci), float("nan"), device=dev, dtype=dtype)
    if Co % (64 if dtype == torch.bfloat16 else 32):          # same channel granularity as szn_conv2d_dgrad: reported
        with pytest.raises(L.SznError):
            L.call("szn_conv2d_dgrad_gemm", C.byref(d), L.ptr(doutd), L.ptr(wG), L.ptr(din), L.stream_ptr())
        return
    L.call("szn_conv2d_dgrad_gemm", C.byref(d), L.ptr(doutd), L.ptr(wG), L.ptr(din), L.stream_ptr())
    assert L.last_kernel() == "col2im_kernel"
    torch.cuda.synchronize()
    tol = 1e-5 if dtype == torch.float32 else 1e-2
    assert relerr(din.float().cpu().permute(0, 3, 1, 2), x.grad) < tol
    # too small a workspace is an error, not a silent fallback
    d.workspace_bytes = nb - 1
    with pytest.raises(L.SznError):
        L.call("szn_conv2d_dgrad_gemm", C.byref(d), L.ptr(doutd), L.ptr(wG), L.ptr(din), L.stream_ptr())


def test_conv_epilogue_scale_and_padded_strides():
    # chan_scale (Dropout2d factors) and out_f32 with a padded output stride (score buffer layout)
    B, Hi, Wi, Ci, Co, ldo = 2, 4, 5, 64, 22, 32
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, Ci, Hi, Wi, generator=g).bfloat16().float()
    w = (torch.randn(Co, Ci, 1, 1, generator=g) / 8).bfloat16().float()
    bias = torch.randn(Co, generator=g)
    scale = (torch.rand(B, Co, generator=g) > 0.5).float() * 2
    ref = F.conv2d(x, w, bias) * scale[:, :, None, None]
    d = L.ConvDesc(L.SZN_BF16, B, Hi, Wi, Ci, Hi, Wi, Co, 1, 1, 0, Ci, ldo, 0, 0, 1)
    out = torch.zeros(B, Hi, Wi, ldo, device="cuda")
    xd, wd, bd, sd = nhwc(x).cuda().bfloat16(), nhwc(w).cuda().bfloat16(), bias.cuda(), scale.cuda()   # keep alive
    L.call("szn_conv2d_fwd", C.byref(d), L.ptr(xd), L.ptr(wd), L.ptr(bd), None, L.ptr(sd), L.ptr(out), L.stream_ptr())
    torch.cuda.synchronize()
    assert relerr(out[..., :Co].cpu().permute(0, 3, 1, 2), ref) < 1e-5
    assert float(out[..., Co:].abs().max()) == 0.0


@pytest.mark.parametrize("geom", [(2, 13, 9, 100), (1, 20, 37, 1), (1, 5, 70, 0)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_conv1_1(dtype, geom):
    B, H, W, pad = geom
    is16 = dtype != torch.float32
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, 3, H, W, generator=g) * 50
    w = torch.randn(64, 3, 3, 3, generator=g) / 5
    bias = torch.randn(64, generator=g)
    x.requires_grad_(False); w.requires_grad_(True)
    pre = F.conv2d(x, w, bias, padding=pad)
    ref = F.relu(pre)
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    dt = L.dtype_code(dtype)
    out = torch.empty(B, Ho, Wo, 64, device="cuda", dtype=dtype)
    wd, xd, bd = nhwc(w.detach()).cuda(), x.cuda(), bias.cuda()   # keep the device tensors alive across the calls
    L.call("szn_conv1_1_fwd", dt, B, H, W, pad, L.ptr(xd), L.ptr(wd), L.ptr(bd), L.ptr(out), L.stream_ptr())
    torch.cuda.synchronize()
    tol = 1e-2 if is16 else 1e-5
    assert relerr(out.float().cpu().permute(0, 3, 1, 2), ref) < tol
    dout = torch.randn(B, 64, Ho, Wo, generator=g)
    if is16:
        dout = dout.to(dtype).float()
    pre.backward(dout)
    dw = torch.empty(64, 3, 3, 3, device="cuda"); db = torch.empty(64, device="cuda")
    doutd = nhwc(dout).cuda().to(dtype)
    ws = torch.empty(L.load().szn_conv1_1_wgrad_workspace_bytes(dt, B, H, W, pad), dtype=torch.uint8, device="cuda")
    L.call("szn_conv1_1_wgrad", dt, B, H, W, pad, L.ptr(xd), L.ptr(doutd), L.ptr(dw), L.ptr(db), 0, L.ptr(ws), L.stream_ptr())
    if is16:     # fused kernel (no im2col image), then the bias-gradient kernel
        assert L.prev_kernel() == "conv1_1_wgrad_reduce", L.prev_kernel()
    torch.cuda.synchronize()
    # 16-bit path: the im2col image is 16-bit (pixel values up to ~150 keep 8 mantissa bits in bf16)
    assert relerr(dw.cpu().permute(0, 3, 1, 2), w.grad) < (1e-2 if is16 else 1e-4)
    assert relerr(db.cpu(), dout.sum((0, 2, 3))) < 1e-4


# Forward only, bit for bit.  Image values are integers in [-4, 4], weights k/4 (|k| <= 8), bias k/8 (|k| <= 16): all exact in bf16 and fp16,
# every product is a multiple of 1/4 and every partial sum of the 27 products plus the bias is a multiple of 1/8 with magnitude
# <= 27 * 4 * 2 + 2 = 218 -- exact in fp32 whatever order the MFMA adds in.  So the kernel must give relu(conv2d), computed in fp32 and
# rounded to the storage type (RNE on both sides), exactly: any slip in the tap decode, the swap pairing or the 8-pixel exchange shows.
#   (17, 130, 130, 1): 17 * 130 * 2 = 4,420 runs for the 4,096 waves of the capped grid -- 324 waves take a second run, all of them touching
#                      the image (the prefetch-then-store hand-over); 9 segments per row = a ragged last run and a ragged last segment
#   (8, 102, 40, 100): 300 x 238 outputs, 4,800 runs, mostly padding: constant-piece stores, runs whose successor does / does not touch the image
#   (1, 5, 70, 0):     small ragged geometry
@pytest.mark.parametrize("geom", [(17, 130, 130, 1), (8, 102, 40, 100), (1, 5, 70, 0)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_conv1_1_fwd_exact(dtype, geom):
    B, H, W, pad = geom
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-4, 5, (B, 3, H, W), generator=g).float()
    w = torch.randint(-8, 9, (64, 3, 3, 3), generator=g).float() / 4
    bias = torch.randint(-16, 17, (64,), generator=g).float() / 8
    ref = nhwc(F.relu(F.conv2d(x, w, bias, padding=pad))).to(dtype)
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    out = torch.empty(B, Ho, Wo, 64, device="cuda", dtype=dtype)
    wd, xd, bd = nhwc(w).cuda(), x.cuda(), bias.cuda()   # keep the device tensors alive across the call
    L.call("szn_conv1_1_fwd", L.dtype_code(dtype), B, H, W, pad, L.ptr(xd), L.ptr(wd), L.ptr(bd), L.ptr(out), L.stream_ptr())
    torch.cuda.synchronize()
    assert L.last_kernel() == "conv1_1_fwd_kernel", L.last_kernel()
    assert torch.equal(out.cpu(), ref)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("hw", [(7, 9), (8, 8), (1, 1), (23, 23)])
def test_maxpool(dtype, hw):
    B, Cc = 2, 64
    Hi, Wi = hw
    g = torch.Generator().manual_seed(11)
    # post-ReLU activations with many exact zeros and ties
    x = F.relu(torch.randn(B, Cc, Hi, Wi, generator=g)).to(dtype).float()
    x = (x * 4).round() / 4
    x.requires_grad_(True)
    ref = F.max_pool2d(x, 2, 2, ceil_mode=True)
    Ho, Wo = ref.shape[2:]
    dt = L.dtype_code(dtype)
    xd = nhwc(x.detach()).cuda().to(dtype)
    out = torch.empty(B, Ho, Wo, Cc, device="cuda", dtype=dtype)
    L.call("szn_maxpool2x2_ceil_fwd", dt, B, Hi, Wi, Cc, L.ptr(xd), L.ptr(out), L.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(out.float().cpu().permute(0, 3, 1, 2), ref.detach())
    dout = torch.randn(B, Cc, Ho, Wo, generator=g).to(dtype).float()
    ref.backward(dout)
    dref = x.grad * (x.detach() > 0)
    din = torch.empty(B, Hi, Wi, Cc, device="cuda", dtype=dtype)
    doutd = nhwc(dout).cuda().to(dtype)
    cs = torch.zeros(Cc, device="cuda")
    L.call("szn_maxpool2x2_ceil_bwd", dt, B, Hi, Wi, Cc, L.ptr(xd), L.ptr(out), L.ptr(doutd), L.ptr(din), L.ptr(cs), None, 0,
           None, L.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(din.float().cpu().permute(0, 3, 1, 2), dref)
    assert relerr(cs.cpu(), dref.sum((0, 2, 3))) < 1e-5          # fused bias gradient = column sums of din
    # deterministic form of the column sums: partial rows + fixed-order reduce
    cs2 = torch.zeros(Cc, device="cuda")
    slab = torch.full((2048 * Cc,), float("nan"), device="cuda")
    ro = L.rows_out()
    L.call("szn_maxpool2x2_ceil_bwd", dt, B, Hi, Wi, Cc, L.ptr(xd), L.ptr(out), L.ptr(doutd), L.ptr(din), L.ptr(cs2), L.ptr(slab),
           2048, C.byref(ro), L.stream_ptr())
    rows = ro.value
    assert 0 < rows <= 2048 and float(cs2.abs().max()) == 0.0
    L.call("szn_colsum_reduce_batch", 1, (C.c_void_p * 1)(slab.data_ptr()), (C.c_int * 1)(rows), (C.c_int * 1)(Cc),
           (C.c_void_p * 1)(cs2.data_ptr()), L.stream_ptr())
    torch.cuda.synchronize()
    assert relerr(cs2.cpu(), dref.sum((0, 2, 3))) < 1e-5
    with pytest.raises(L.SznError):
        L.call("szn_maxpool2x2_ceil_bwd", dt, B, Hi, Wi, Cc, L.ptr(xd), L.ptr(out), L.ptr(doutd), L.ptr(din), L.ptr(cs2), L.ptr(slab),
               0, C.byref(ro), L.stream_ptr())
    assert ro.value == 0                                          # a refused call reports no rows


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_gemm_proj_aliases_and_cast(dt):
    """the "pixel projection" entry points of the C-ABI (szn_gemm_proj_fwd / dgrad / wgrad: score_fr as a plain
    (M x 4096) x (4096 x N) GEMM, models.py:93,145) and szn_cast, against torch matmul on the same rounded operands"""
    M, K, N = 2 * 17 * 17, 4096, 300
    ldo = 304
    code = L.dtype_code(dt)
    g = torch.Generator(device="cuda").manual_seed(23)
    x32 = torch.randn(M, K, device="cuda", generator=g)
    w32 = torch.randn(N, K, device="cuda", generator=g) / K ** 0.5
    bias = torch.randn(N, device="cuda", generator=g)
    x = torch.empty(M, K, device="cuda", dtype=dt)
    w = torch.empty(N, K, device="cuda", dtype=dt)
    st = L.stream_ptr()
    L.call("szn_cast", L.SZN_F32, code, M * K, L.ptr(x32), L.ptr(x), st)
    L.call("szn_cast", L.SZN_F32, code, N * K, L.ptr(w32), L.ptr(w), st)
    assert torch.equal(x, x32.to(dt)) and torch.equal(w, w32.to(dt))           # round-to-nearest-even like torch
    back = torch.empty(M, K, device="cuda")
    L.call("szn_cast", code, L.SZN_F32, M * K, L.ptr(x), L.ptr(back), st)
    assert torch.equal(back, x.float())
    tol = 1e-4 if dt == torch.float32 else 2e-3
    out = torch.zeros(M, ldo, device="cuda")
    L.call("szn_gemm_proj_fwd", code, M, K, N, ldo, L.ptr(x), L.ptr(w), L.ptr(bias), L.ptr(out), st)
    ref = x.double() @ w.double().t() + bias.double()
    assert float((out[:, :N].double() - ref).abs().max() / ref.abs().max()) < tol
    # wgrad: dW = dout^T @ x (dout rows padded to ldo)
    dout = torch.zeros(M, ldo, device="cuda", dtype=dt)
    dout[:, :N] = torch.randn(M, N, device="cuda", generator=g).to(dt)
    dw = torch.empty(N, K, device="cuda")
    L.call("szn_gemm_proj_wgrad", code, M, K, N, ldo, L.ptr(x), L.ptr(dout), L.ptr(dw), 0, st)
    ref_dw = dout[:, :N].double().t() @ x.double()
    assert float((dw.double() - ref_dw).abs().max() / ref_dw.abs().max()) < tol
    # dgrad: dx = dout @ W with the ReLU gate of x, on the 64-padded head width the engine uses (zero rows behind N)
    NP = 320
    wp = torch.zeros(NP, K, device="cuda", dtype=dt)
    wp[:N] = w
    dp = torch.zeros(M, NP, device="cuda", dtype=dt)
    dp[:, :N] = dout[:, :N]
    wT = torch.empty(K, NP, device="cuda", dtype=dt)
    L.call("szn_pack_weight_dgrad", code, NP, 1, 1, K, L.ptr(wp), L.ptr(wT), st)
    dx = torch.empty(M, K, device="cuda", dtype=dt)
    L.call("szn_gemm_proj_dgrad", code, M, K, NP, NP, L.ptr(dp), L.ptr(wT), L.ptr(x), None, L.ptr(dx), st)
    ref_dx = (dout[:, :N].double() @ w.double()) * (x.double() > 0)
    assert float((dx.double() - ref_dx).abs().max() / ref_dx.abs().max()) < (1e-4 if dt == torch.float32 else 1e-2)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M,out32,N", [(65536 + 77, False, 300), (4 * 65536, True, 300), (65536, True, 304), (65536 + 8, False, 320)])
def test_proj_gemm_stream(dt, M, out32, N):
    """the HBM-streaming projection kernel (proj_gemm_stream: M x 4096 x 300 with >= 256 pixel tiles -- the full-resolution
    "H*W x 300" shape of the north star) through szn_gemm_proj_fwd, against torch matmul on the same rounded operands; a ragged
    last tile, padded output rows, 16-bit and fp32 output, 19 and 20 cout fragments (N <= 304 / N = 320); run-to-run bit-identical"""
    K = 4096
    ldo = 328 if out32 else (N + 7) // 8 * 8 + 8
    code = L.dtype_code(dt)
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.relu(torch.randn(M, K, device="cuda", generator=g)).to(dt)           # fc7's output is post-ReLU
    w = (torch.randn(N, K, device="cuda", generator=g) / K ** 0.5).to(dt)
    bias = torch.randn(N, device="cuda", generator=g)
    st = L.stream_ptr()
    outs = []
    for _ in range(2):
        out = torch.full((M, ldo), 7.0, device="cuda", dtype=torch.float32 if out32 else dt)
        d = L.ConvDesc(code, 1, 1, M, K, 1, M, N, 1, 1, 0, K, ldo, 0, 0, int(out32))
        L.call("szn_conv2d_fwd", C.byref(d), L.ptr(x), L.ptr(w), L.ptr(bias), None, None, L.ptr(out), st)
        torch.cuda.synchronize()
        assert L.last_kernel() == "proj_gemm_stream"
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    assert bool((outs[0][:, N:] == 7.0).all())                                   # the padding columns are not touched
    worst = 0.0
    for s in range(0, M, 65536):                                                 # reference in slices (fp32 matmul on the GPU)
        ref = x[s:s + 65536].float() @ w.float().t() + bias
        got = outs[0][s:s + 65536, :N].float()
        worst = max(worst, float((got - ref).abs().max() / ref.abs().max()))
    assert worst < (2e-4 if out32 else 6e-3), worst


_PROBE_SHAPES = [(2, 47, 256, 256, 3, 1), (8, 89, 128, 256, 3, 1), (8, 17, 512, 4096, 1, 0), (2, 45, 512, 128, 3, 1), (1, 33, 64, 320, 1, 0)]
# 256-wide tile shapes with >= 240 tiles: 3x3 forward + dgrad (gate, column sums), a 1x1 with a Dropout2d factor, ragged pixel tiles
_PROBE_SHAPES_8PH = [(8, 89, 256, 256, 3, 1), (3, 150, 64, 256, 3, 1), (4, 131, 256, 512, 1, 0), (2, 181, 256, 256, 5, 2), (1, 260, 128, 256, 3, 1)]
_EPILOGUE_PROBE = r'''
import ctypes as C, hashlib, sys, torch
sys.path.insert(0, %r)
from zeroshotsemanticsegmentation_amd import _lib as L
torch.manual_seed(7)
dt = L.dtype_code(torch.bfloat16)
out_lines = []
# (B, Hi, Ci, Co, K, pad): wide_rows (3x3, 256 couts), igemm_wide 192-tiles (1x1, few tiles), igemm_v2 (128 couts), ragged sizes
for (B, Hi, Ci, Co, K, pad) in %s:
    Ho = Hi + 2 * pad - K + 1
    x = torch.randn(B, Hi, Hi, Ci, device="cuda").bfloat16()
    w = (torch.randn(Co, K, K, Ci, device="cuda") / (Ci * K * K) ** 0.5).bfloat16()
    bias = torch.randn(Co, device="cuda")
    gate = torch.relu(torch.randn(B, Hi, Hi, Ci, device="cuda")).bfloat16()
    scale = (torch.rand(B, Co, device="cuda") > 0.5).float() * 2
    out = torch.zeros(B, Ho, Ho, Co, device="cuda", dtype=torch.bfloat16)
    d = L.ConvDesc(dt, B, Hi, Hi, Ci, Ho, Ho, Co, K, K, pad, Ci, Co, Ci, 1, 0)
    L.call("szn_conv2d_fwd", C.byref(d), L.ptr(x), L.ptr(w), L.ptr(bias), None, L.ptr(scale) if K == 1 else None, L.ptr(out), L.stream_ptr())
    k1 = L.last_kernel()
    wT = torch.empty(Ci, K, K, Co, device="cuda", dtype=torch.bfloat16)
    L.call("szn_pack_weight_dgrad", dt, Co, K, K, Ci, L.ptr(w), L.ptr(wT), L.stream_ptr())
    dout = torch.randn(B, Ho, Ho, Co, device="cuda").bfloat16()
    din = torch.zeros(B, Hi, Hi, Ci, device="cuda", dtype=torch.bfloat16)
    cs = torch.zeros(Ci, device="cuda"); slab = torch.zeros(4096, Ci, device="cuda")
    d2 = L.ConvDesc(dt, B, Hi, Hi, Ci, Ho, Ho, Co, K, K, pad, Ci, Co, Ci, 0, 0)
    d2.colsum, d2.colsum_slab, d2.colsum_slab_rows = cs.data_ptr(), slab.data_ptr(), 4096
    L.call("szn_conv2d_dgrad", C.byref(d2), L.ptr(dout), L.ptr(wT), L.ptr(gate), None, L.ptr(din), L.stream_ptr())
    k2 = L.last_kernel()
    torch.cuda.synchronize()
    h = hashlib.sha256(out.view(torch.int16).cpu().numpy().tobytes() + din.view(torch.int16).cpu().numpy().tobytes()).hexdigest()
    out_lines.append("%%s %%s %%s %%.6e %%.6e %%.6e" %% (h, k1, k2, float(slab.sum()), float(out.float().abs().sum()), float(din.float().abs().sum())))
print("\n".join(out_lines))
'''


def test_register_epilogue_equals_the_staged_epilogue_bit_for_bit():
    """the epilogue from the accumulator registers (szn_epilogue.h) and the LDS-staged one it replaced write the same bits
    (forward: bias + ReLU (+ Dropout2d factor); dgrad: gate + column sums, whose ORDER differs: compared to 1e-5)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    runs = {}
    # (SZN_WIDE_8PH=0: the round 1-3 tile kernels, which have both epilogues; conv_igemm_8ph has the register epilogue only and is
    # compared with them in test_8phase_kernel_equals_conv_igemm_wide_bit_for_bit)
    for tag, env in (("direct", {"SZN_WIDE_8PH": "0"}),
                     ("staged", {"SZN_WIDE_8PH": "0", "SZN_WIDE_DIRECT": "0", "SZN_IGEMM_DIRECT": "0"})):
        e = dict(os.environ); e.update(env)
        r = subprocess.run([sys.executable, "-c", _EPILOGUE_PROBE % (root, _PROBE_SHAPES)], env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        runs[tag] = [ln.split() for ln in r.stdout.strip().splitlines() if len(ln.split()) == 6]
    assert len(runs["direct"]) == 5 and len(runs["staged"]) == 5, (runs,)
    kernels = set()
    for a, b in zip(runs["direct"], runs["staged"]):
        assert a[0] == b[0], (a, b)                      # outputs + input gradients: same bits
        assert a[1] == b[1] and a[2] == b[2], (a, b)     # same kernels picked
        assert abs(float(a[3]) - float(b[3])) <= 1e-5 * max(1.0, abs(float(b[3]))), (a, b)
        kernels.update((a[1], a[2]))
    assert {"conv3x3_wide_rows", "conv_igemm_wide", "conv_igemm_v2"} <= kernels, kernels


def test_8phase_kernel_equals_conv_igemm_wide_bit_for_bit():
    """conv_igemm_8ph (round 4: the 8-phase schedule on 256 x 256 tiles; its 128-cout form was removed in round 6) accumulates every output element over the same K order
    (tap, cin chunk, two K halves) as conv_igemm_wide / conv_igemm_v2, so the kernels must write the same bits -- forward (bias, ReLU, Dropout2d factor) and dgrad
    (gate; column sums to rounding: another grouping).  The probe runs each kernel set in its own process (the switch is read once)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    runs = {}
    # (SZN_8PH_KORD=0: the tap-major K order of the kernels it is compared with; the shipped default walks the K tiles cin-chunk-major --
    # other summation order, same sums: third run, compared by value)
    for tag, env in (("8ph", {"SZN_8PH_KORD": "0"}), ("wide", {"SZN_WIDE_8PH": "0", "SZN_WIDE_ROWS": "0"}),
                     ("8ph_chunk_major", {"SZN_8PH_KORD": "1"})):
        e = dict(os.environ); e.update(env)
        r = subprocess.run([sys.executable, "-c", _EPILOGUE_PROBE % (root, _PROBE_SHAPES_8PH)], env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        runs[tag] = [ln.split() for ln in r.stdout.strip().splitlines() if len(ln.split()) == 6]
    assert len(runs["8ph"]) == 5 and len(runs["wide"]) == 5 and len(runs["8ph_chunk_major"]) == 5, (runs,)
    differs = 0
    for a, c in zip(runs["8ph"], runs["8ph_chunk_major"]):
        assert a[1] == c[1] and a[2] == c[2], (a, c)
        differs += a[0] != c[0]
        for i in (3, 4, 5):                              # column sums, sum |out|, sum |din|: a handful of 16-bit roundings apart
            assert abs(float(a[i]) - float(c[i])) <= 2e-5 * max(1.0, abs(float(a[i]))), (a, c)
    assert differs >= 3, runs                            # (K > 1 shapes really take the other order; the 1x1 shape has one order)
    seen = 0
    for a, b in zip(runs["8ph"], runs["wide"]):
        assert a[0] == b[0], (a, b)                      # outputs + input gradients: same bits
        assert abs(float(a[3]) - float(b[3])) <= 1e-5 * max(1.0, abs(float(b[3]))), (a, b)
        for ka, kb in ((a[1], b[1]), (a[2], b[2])):
            if ka.startswith("conv_igemm_8ph"):
                seen += 1
                assert kb == "conv_igemm_wide", (a, b)
            else:
                assert ka == kb, (a, b)
    assert seen >= 6, runs


@pytest.mark.parametrize("geom", [(8, 23, 512, 1024, 7), (4, 28, 128, 128, 5), (1, 23, 512, 1024, 7), (1, 25, 512, 256, 7)])
def test_dgrad_gemm_on_the_forward_weight_layout(geom):
    """szn_conv2d_dgrad_gemm_native (GEMM on the filter bank as the forward pass stores it, dout transposed instead) ==
    szn_conv2d_dgrad_gemm on the packed transpose, to fp32 accumulation order, and both == torch"""
    B, Hi, Ci, Co, K = geom
    Ho = Hi - K + 1
    g = torch.Generator().manual_seed(9)
    w = (torch.randn(Co, Ci, K, K, generator=g) / (Ci * K * K) ** 0.5).bfloat16().float()
    dout = torch.randn(B, Co, Ho, Ho, generator=g).bfloat16().float()
    ref = torch.nn.grad.conv2d_input((B, Ci, Hi, Hi), w, dout)
    dt = L.dtype_code(torch.bfloat16)
    wd, dd = nhwc(w).cuda().bfloat16(), nhwc(dout).cuda().bfloat16()
    N = K * K * Ci
    d = L.ConvDesc(dt, B, Hi, Hi, Ci, Ho, Ho, Co, K, K, 0, Ci, Co, 0, 0, 0)
    lib = L.load()
    assert lib.szn_conv2d_dgrad_gemm_native_supported(C.byref(d)) == 1
    ws = torch.empty(lib.szn_conv2d_dgrad_gemm_native_workspace_bytes(C.byref(d)), dtype=torch.uint8, device="cuda")
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    din = torch.empty(B, Hi, Hi, Ci, device="cuda", dtype=torch.bfloat16)
    L.call("szn_conv2d_dgrad_gemm_native", C.byref(d), L.ptr(dd), L.ptr(wd), L.ptr(din), L.stream_ptr())
    assert L.last_kernel() == "col2im_kernel" and L.prev_kernel() == "conv_wgrad_wide", (L.prev_kernel(), L.last_kernel())
    torch.cuda.synchronize()
    wG = torch.empty(N, Co, device="cuda", dtype=torch.bfloat16)
    L.call("szn_pack_weight_dgrad", dt, Co, 1, 1, N, L.ptr(wd), L.ptr(wG), L.stream_ptr())
    din2 = torch.empty_like(din)
    L.call("szn_conv2d_dgrad_gemm", C.byref(d), L.ptr(dd), L.ptr(wG), L.ptr(din2), L.stream_ptr())
    torch.cuda.synchronize()
    a, b2 = din.float().cpu().permute(0, 3, 1, 2), din2.float().cpu().permute(0, 3, 1, 2)
    assert relerr(a, ref) < 1e-2 and relerr(b2, ref) < 1e-2
    assert relerr(a, b2) < 4e-3                       # both round the same fp32 sums (different order) to bf16
    # a shape the two-K-major kernel does not take (too few pixels): the caller has to use the packed form
    d3 = L.ConvDesc(dt, 1, 8, 8, 64, 2, 2, 256, 7, 7, 0, 64, 256, 0, 0, 0)
    assert lib.szn_conv2d_dgrad_gemm_native_supported(C.byref(d3)) == 0


@pytest.mark.parametrize("case", [(2, 262, 262, 64, 64, (98, 164), (0, 262)), (1, 355, 355, 128, 128, (48, 308), (2, 353)),
                                  (2, 200, 230, 64, 128, (40, 120), (1, 199)), (1, 710, 710, 64, 64, (98, 612), (0, 710))])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_wgrad_constant_border_hint_equals_dense(case, dtype):
    """szn_conv2d_wgrad with the constant-border hint (tiles whose whole input patch is one value per channel are replaced by a
    rank-one term: column sum of dout x that value) against the same call without the hint: the same sums in a different fp32 order"""
    B, H, W, Ci, Co, rect, const = case
    g = torch.Generator().manual_seed(31)
    x = torch.relu(torch.randn(B, H, W, Ci, generator=g))
    cval = torch.relu(torch.randn(Ci, generator=g)) + 0.25
    # constant outside rect (inside const); the frame outside const holds other values again (what zero padding does to a layer)
    inside = torch.zeros(H, W, dtype=torch.bool)
    inside[rect[0]:rect[1], rect[0]:rect[1]] = True
    frame = torch.ones(H, W, dtype=torch.bool)
    frame[const[0]:const[1], const[0]:min(const[1], W)] = False
    x = torch.where((inside | frame)[None, :, :, None], x, cval[None, None, None, :].expand(B, H, W, Ci)).to(dtype).cuda()
    dout = (torch.randn(B, H, W, Co, generator=g) * 0.1).to(dtype).cuda()
    dt = L.dtype_code(dtype)
    ws = torch.empty(2 * 256 * 64 * 9 * 64 * 4, dtype=torch.uint8, device="cuda")

    def run(hint):
        d = L.ConvDesc(dt, B, H, W, Ci, H, W, Co, 3, 3, 1, Ci, Co, 0, 0, 0)
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
        if hint:
            d.cb_on = 1
            d.cb_rect[0], d.cb_rect[1], d.cb_rect[2], d.cb_rect[3] = rect[0], rect[1], rect[0], rect[1]
            d.cb_const[0], d.cb_const[1], d.cb_const[2], d.cb_const[3] = const[0], const[1], const[0], min(const[1], W)
        dw = torch.full((Co, 3, 3, Ci), 7.0, device="cuda")
        L.call("szn_conv2d_wgrad", C.byref(d), L.ptr(x), L.ptr(dout), L.ptr(dw), 0, L.stream_ptr())
        torch.cuda.synchronize()
        return dw, L.last_kernel(), d.res.work_fraction

    dense, k0, f0 = run(False)
    hinted, k1, f1 = run(True)
    assert k0 == "wgrad_taps_reduce" and k1 == "wgrad_taps_reduce"
    assert f1 < 0.95 or B * (H // 16) * (W // 16) < 600, f1    # tiles were really skipped (small maps: too few would be left, dense run)
    err = float((hinted - dense).abs().max() / dense.abs().max())
    assert err < 1e-5, err
    again, _, _ = run(True)
    assert torch.equal(again, hinted)                     # fixed-order sums: bit-reproducible
    # accumulate != 0 ignores the hint (documented): the dense sum on top of what is there
    d = L.ConvDesc(dt, B, H, W, Ci, H, W, Co, 3, 3, 1, Ci, Co, 0, 0, 0)
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    d.cb_on = 1
    d.cb_rect[0], d.cb_rect[1], d.cb_rect[2], d.cb_rect[3] = rect[0], rect[1], rect[0], rect[1]
    d.cb_const[0], d.cb_const[1], d.cb_const[2], d.cb_const[3] = const[0], const[1], const[0], min(const[1], W)
    acc = dense.clone()
    L.call("szn_conv2d_wgrad", C.byref(d), L.ptr(x), L.ptr(dout), L.ptr(acc), 1, L.stream_ptr())
    torch.cuda.synchronize()
    assert float((acc - 2 * dense).abs().max() / dense.abs().max()) < 1e-6


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_pool_backward_sums_the_tiles_the_weight_gradient_skips(dtype):
    """szn_conv2d_wgrad_cb_region names the pixels (whole 16 x 16 tiles) a hinted weight-gradient call replaces by a rank-one term;
    szn_maxpool2x2_ceil_bwd_code_cb sums its output over exactly those tiles while writing it (same din, same bias sums as the plain
    call), and the weight gradient that is handed the sum equals the one that sums for itself and the dense one"""
    B, H, W, Ci, Co = 2, 710, 710, 64, 64
    rect, const = (98, 612), (0, 710)
    g = torch.Generator().manual_seed(41)
    x = torch.relu(torch.randn(B, H, W, Ci, generator=g))
    cval = torch.relu(torch.randn(Ci, generator=g)) + 0.25
    inside = torch.zeros(H, W, dtype=torch.bool)
    inside[rect[0]:rect[1], rect[0]:rect[1]] = True
    x = torch.where(inside[None, :, :, None], x, cval[None, None, None, :].expand(B, H, W, Ci)).to(dtype).cuda()
    Hp = (H + 1) // 2
    dpool = (torch.randn(B, Hp, Hp, Co, generator=g) * 0.1).to(dtype).cuda()
    code = torch.randint(0, 5, (B, Hp, Hp, Co), generator=g, dtype=torch.uint8).cuda()
    dt = L.dtype_code(dtype)
    lib = L.load()
    ws = torch.empty(2 * 256 * 64 * 9 * 64 * 4, dtype=torch.uint8, device="cuda")

    def desc(hint):
        d = L.ConvDesc(dt, B, H, W, Ci, H, W, Co, 3, 3, 1, Ci, Co, 0, 0, 0)
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
        if hint:
            d.cb_on = 1
            d.cb_rect[0], d.cb_rect[1], d.cb_rect[2], d.cb_rect[3] = rect[0], rect[1], rect[0], rect[1]
            d.cb_const[0], d.cb_const[1], d.cb_const[2], d.cb_const[3] = const[0], const[1], const[0], const[1]
        return d

    tiles = (C.c_int * 8)()
    assert lib.szn_conv2d_wgrad_cb_region(C.byref(desc(True)), tiles) == 1
    assert lib.szn_conv2d_wgrad_cb_region(C.byref(desc(False)), tiles) == 0
    assert all(v % 16 == 0 for v in tiles)
    fy0, fy1, fx0, fx1, wy0, wy1, wx0, wx1 = [v // 16 for v in tiles]
    assert 0 < fy0 < wy0 < wy1 < fy1 <= H // 16
    rows = 512
    st = L.stream_ptr()
    din0, din1 = torch.empty(B, H, W, Co, device="cuda", dtype=dtype), torch.empty(B, H, W, Co, device="cuda", dtype=dtype)
    cs0, cs1 = torch.zeros(Co, device="cuda"), torch.zeros(Co, device="cuda")
    slab0, slab1, slab2 = (torch.zeros(rows * Co, device="cuda") for _ in range(3))
    ssum = torch.full((Co,), 7.0, device="cuda")
    ro0, ro1 = L.rows_out(), L.rows_out()
    L.call("szn_maxpool2x2_ceil_bwd_code", dt, B, H, W, Co, L.ptr(code), L.ptr(dpool), L.ptr(din0), L.ptr(cs0), L.ptr(slab0), rows, C.byref(ro0), st)
    L.call("szn_maxpool2x2_ceil_bwd_code_cb", dt, B, H, W, Co, L.ptr(code), L.ptr(dpool), L.ptr(din1), L.ptr(cs1), L.ptr(slab1), rows,
           C.byref(ro1), tiles, 1, L.ptr(ssum), L.ptr(slab2), st)
    assert 0 < ro0.value == ro1.value <= rows
    assert L.last_kernel() == "slab_rows_sum_kernel" and L.prev_kernel() == "maxpool_bwd_code_kernel"
    torch.cuda.synchronize()
    assert torch.equal(din0, din1) and torch.equal(slab0, slab1)
    mask = torch.zeros(H, W, dtype=torch.bool, device="cuda")
    mask[16 * fy0:16 * fy1, 16 * fx0:16 * fx1] = True
    mask[16 * wy0:16 * wy1, 16 * wx0:16 * wx1] = False
    want = (din0.double() * mask[None, :, :, None]).sum(dim=(0, 1, 2))
    assert float((ssum.double() - want).abs().max() / want.abs().max()) < 1e-5
    # the three forms of the weight gradient
    def wgrad(d):
        dw = torch.empty(Co, 3, 3, Ci, device="cuda")
        L.call("szn_conv2d_wgrad", C.byref(d), L.ptr(x), L.ptr(din0), L.ptr(dw), 0, st)
        torch.cuda.synchronize()
        return dw, L.prev_kernel()
    dense, _ = wgrad(desc(False))
    own, k_own = wgrad(desc(True))
    dh = desc(True)
    dh.colsum = ssum.data_ptr()
    given, k_given = wgrad(dh)
    assert k_own == "wgrad_cb_colsum" and k_given == "conv_wgrad_taps"       # (the launch in front of wgrad_taps_reduce)
    scale = float(dense.abs().max())
    assert float((own - dense).abs().max()) / scale < 1e-5 and float((given - dense).abs().max()) / scale < 1e-5
    assert float((given - own).abs().max()) / scale < 1e-6


@pytest.mark.parametrize("case", [(2, 710, 710, (98, 612), (97, 613)), (1, 262, 262, (98, 164), (96, 166)), (2, 355, 300, (48, 200), (40, 210)),
                                  (1, 710, 710, (2, 708), (1, 709))])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_dgrad_border_tiles_replaced_by_region_sums(case, dtype):
    """szn_conv2d_dgrad with cb_on == 2 does not run the tiles that neither store anything nor see a varying gate;
    szn_conv2d_dgrad_border_finish adds their share of the column sums from the sum of dout outside
    szn_conv2d_dgrad_border_region()'s rectangle + 1-pixel strips it reads itself.  Against the same call with cb_on == 1 (every tile
    run): din bit-equal where it is read, column sums equal to fp32 summation order; the region sum also through the pool's backward pass"""
    B, H, W, grect, srect = case
    Ci = Co = 64
    g = torch.Generator().manual_seed(51)
    gate = torch.randn(B, H, W, Ci, generator=g)                              # conv1_1's output: ReLU'd later = the gate is (gate > 0)
    gconst = torch.randn(Ci, generator=g)
    ins = torch.zeros(H, W, dtype=torch.bool)
    ins[grect[0]:grect[1], grect[0]:min(grect[1], W)] = True
    gate = torch.where(ins[None, :, :, None], gate, gconst[None, None, None, :].expand(B, H, W, Ci)).to(dtype).cuda()
    Hp, Wp = (H + 1) // 2, (W + 1) // 2
    dpool = (torch.randn(B, Hp, Wp, Co, generator=g) * 0.1).to(dtype).cuda()
    code = torch.randint(0, 5, (B, Hp, Wp, Co), generator=g, dtype=torch.uint8).cuda()
    wT = (torch.randn(Ci, 3, 3, Co, generator=g) / 24.0).to(dtype).cuda()
    dt = L.dtype_code(dtype)
    lib = L.load()
    st = L.stream_ptr()

    def desc(mode):
        d = L.ConvDesc(dt, B, H, W, Ci, H, W, Co, 3, 3, 1, Ci, Co, Ci, 0, 0)
        d.cb_on = mode
        d.cb_rect[0], d.cb_rect[1], d.cb_rect[2], d.cb_rect[3] = grect[0], grect[1], grect[0], min(grect[1], W)
        d.cb_const[0], d.cb_const[1], d.cb_const[2], d.cb_const[3] = srect[0], srect[1], srect[0], min(srect[1], W)
        return d

    region = (C.c_int * 8)()
    has = lib.szn_conv2d_dgrad_border_region(C.byref(desc(2)), region)
    assert lib.szn_conv2d_dgrad_border_region(C.byref(desc(1)), region) == 0
    if grect == (2, 708):
        assert has == 0                                                    # (everything is read: nothing to skip)
        return
    assert has == 1
    r = list(region)
    assert r[0] == 0 and r[1] == H and r[2] == 0 and r[3] == W and r[4] <= min(grect[0], srect[0]) and r[5] >= min(max(grect[1], srect[1]), H)
    # dout through the pool's backward pass, which also sums it outside the rectangle
    rows = 512
    dout = torch.empty(B, H, W, Co, device="cuda", dtype=dtype)
    cs, slab = torch.zeros(Co, device="cuda"), torch.zeros(rows * Co, device="cuda")
    ssum, slab2 = torch.full((1, Co), 7.0, device="cuda"), torch.zeros(rows * Co, device="cuda")
    even = all(v % 2 == 0 for v in r)
    if even:
        L.call("szn_maxpool2x2_ceil_bwd_code_cb", dt, B, H, W, Co, L.ptr(code), L.ptr(dpool), L.ptr(dout), L.ptr(cs), L.ptr(slab), rows,
               None, region, 1, L.ptr(ssum), L.ptr(slab2), st)
    else:
        L.call("szn_maxpool2x2_ceil_bwd_code", dt, B, H, W, Co, L.ptr(code), L.ptr(dpool), L.ptr(dout), L.ptr(cs), L.ptr(slab), rows, None, st)
    torch.cuda.synchronize()
    mask = torch.ones(H, W, dtype=torch.bool, device="cuda")
    mask[r[4]:r[5], r[6]:r[7]] = False
    want = (dout.double() * mask[None, :, :, None]).sum(dim=(0, 1, 2))
    if even:
        assert float((ssum[0].double() - want).abs().max() / want.abs().max()) < 1e-5
    s0 = want.float().contiguous()

    def run(mode):
        d = desc(mode)
        din = torch.full((B, H, W, Ci), 3.0, device="cuda", dtype=dtype)
        colsum = torch.zeros(Ci, device="cuda")
        d.colsum = colsum.data_ptr()
        L.call("szn_conv2d_dgrad", C.byref(d), L.ptr(dout), L.ptr(wT), L.ptr(gate), None, L.ptr(din), st)
        frac = d.res.work_fraction
        kern = L.last_kernel()
        if mode == 2:
            assert frac < 0.95
            ws = torch.empty(2 * 24 * B * Co, device="cuda")
            L.call("szn_conv2d_dgrad_border_finish", C.byref(d), L.ptr(dout), L.ptr(wT), L.ptr(gate), L.ptr(s0), L.ptr(colsum), L.ptr(ws), st)
        torch.cuda.synchronize()
        return din, colsum, kern

    din1, cs1, k1 = run(1)
    din2, cs2, k2 = run(2)
    assert k1 == "conv3x3_regw" and k2 == "conv3x3_regw"
    sy0, sy1, sx0, sx1 = srect[0], min(srect[1], H), srect[0], min(srect[1], W)
    assert torch.equal(din1[:, sy0:sy1, sx0:sx1], din2[:, sy0:sy1, sx0:sx1])
    # the reference value of the column sums: the dense gated dgrad in float64
    x64 = dout.double().permute(0, 3, 1, 2)
    w64 = wT.double().permute(0, 3, 1, 2)                                   # [Ci][Co][3][3]: din = conv(dout, wT), pad 1
    ref = (torch.nn.functional.conv2d(x64.cpu(), w64.cpu(), padding=1) * (gate.double().permute(0, 3, 1, 2).cpu() > 0)).sum(dim=(0, 2, 3))
    scale = float(ref.abs().max())
    assert float((cs1.double().cpu() - ref).abs().max()) / scale < 2e-4      # (the kernel rounds din to 16 bits before it sums it)
    assert float((cs2 - cs1).abs().max()) / scale < 2e-4
    # tighter: the skipped part alone against float64 (no 16-bit rounding on either side)
    m64 = mask.cpu()[None, None].double()
    ref_skip = (torch.nn.functional.conv2d(x64.cpu(), w64.cpu(), padding=1) * (gate.double().permute(0, 3, 1, 2).cpu() > 0) * m64).sum(dim=(0, 2, 3))
    ran = torch.zeros(Ci, device="cuda")
    d = desc(2)
    d.colsum = ran.data_ptr()
    dinx = torch.empty(B, H, W, Ci, device="cuda", dtype=dtype)
    L.call("szn_conv2d_dgrad", C.byref(d), L.ptr(dout), L.ptr(wT), L.ptr(gate), None, L.ptr(dinx), st)
    torch.cuda.synchronize()
    got_skip = (cs2 - ran).double().cpu()
    assert float((got_skip - ref_skip).abs().max()) / float(ref_skip.abs().max() + 1e-30) < 1e-4


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("geom", [(2, 37, 41, 64, 64), (1, 710, 64, 64, 64), (2, 45, 45, 512, 512)])
def test_pool_winner_codes(dtype, geom):
    """conv + fused / unfused MaxPool2d(2,2,ceil) with winner codes: codes == first maximum of the stored window (4 = not positive),
    pool_only leaves the pooled tensor and the codes unchanged, and szn_maxpool2x2_ceil_bwd_code == szn_maxpool2x2_ceil_bwd bit for bit"""
    B, Hi, Wi, Ci, Co = geom
    if dtype == torch.float32 and Hi > 100:
        pytest.skip("large fp32 case not needed")
    g = torch.Generator().manual_seed(21)
    x = torch.relu(torch.randn(B, Hi, Wi, Ci, generator=g)).cuda().to(dtype)
    w = (torch.randn(Co, 3, 3, Ci, generator=g) / (Ci * 9) ** 0.5).cuda().to(dtype)
    bias = torch.randn(Co, generator=g).cuda()
    dt = L.dtype_code(dtype)
    Hp, Wp = (Hi + 1) // 2, (Wi + 1) // 2
    res = []
    for pool_only in (0, 1):
        out = torch.full((B, Hi, Wi, Co), 7.0, device="cuda", dtype=dtype)
        pool = torch.empty(B, Hp, Wp, Co, device="cuda", dtype=dtype)
        code = torch.full((B, Hp, Wp, Co), 9, device="cuda", dtype=torch.uint8)
        d = L.ConvDesc(dt, B, Hi, Wi, Ci, Hi, Wi, Co, 3, 3, 1, Ci, Co, 0, 1, 0)
        d.pool_out, d.pool_code, d.pool_only = pool.data_ptr(), code.data_ptr(), pool_only
        L.call("szn_conv2d_fwd", C.byref(d), L.ptr(x), L.ptr(w), L.ptr(bias), None, None, L.ptr(out), L.stream_ptr())
        torch.cuda.synchronize()
        res.append((out, pool, code))
    out, pool, code = res[0]
    assert torch.equal(res[1][1], pool) and torch.equal(res[1][2], code)
    # reference codes from the stored un-pooled tensor
    xo = out.float().permute(0, 3, 1, 2)
    pad = torch.nn.functional.pad(xo, (0, 2 * Wp - Wi, 0, 2 * Hp - Hi), value=-1.0)          # out-of-range members never win
    win = pad.unfold(2, 2, 2).unfold(3, 2, 2).reshape(B, Co, Hp, Wp, 4)
    mx, arg = win.max(dim=-1)
    first = (win == mx.unsqueeze(-1)).float().argmax(dim=-1)                                # first maximum in scan order
    want = torch.where(mx > 0, first, torch.full_like(first, 4)).permute(0, 2, 3, 1).to(torch.uint8)
    assert torch.equal(pool.float().permute(0, 3, 1, 2), mx)
    assert torch.equal(code, want)
    # backward: from the codes == from the tensor
    dp = torch.randn(B, Hp, Wp, Co, generator=g).cuda().to(dtype)
    outs = []
    for use_code in (False, True):
        din = torch.empty(B, Hi, Wi, Co, device="cuda", dtype=dtype)
        cs = torch.zeros(Co, device="cuda"); slab = torch.zeros(512, Co, device="cuda")
        if use_code:
            L.call("szn_maxpool2x2_ceil_bwd_code", dt, B, Hi, Wi, Co, L.ptr(code), L.ptr(dp), L.ptr(din), L.ptr(cs), L.ptr(slab), 512,
                   None, L.stream_ptr())
        else:
            L.call("szn_maxpool2x2_ceil_bwd", dt, B, Hi, Wi, Co, L.ptr(out), L.ptr(pool), L.ptr(dp), L.ptr(din), L.ptr(cs), L.ptr(slab), 512,
                   None, L.stream_ptr())
        torch.cuda.synchronize()
        outs.append((din, slab.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert float(outs[0][0].float().abs().sum()) > 0


@pytest.mark.parametrize("case", [("conv1_2", 2, 710, 64, 64, (97, 613, 1, 709)), ("conv2_1", 2, 355, 64, 128, (47, 308, 2, 353)),
                                  ("conv2_2", 2, 355, 128, 128, (46, 309, 3, 352)), ("ragged", 1, 300, 64, 64, (60, 200, 1, 299))])
def test_constant_border_hint_is_bit_exact(case):
    """szn_conv_desc_t.cb_on: conv3x3_regw runs the tiles the image / the zero padding can reach and broadcasts one computed pixel to
    the others -- out, pool_out and pool_code are the same bits as the dense run (input: constant outside the previous layer's rectangle)"""
    name, B, Hi, Ci, Co, reg = case
    g = torch.Generator().manual_seed(31)
    dt = L.dtype_code(torch.bfloat16)
    r0, r1, c0, c1 = reg                                  # this conv's OUTPUT regions (same on both axes)
    # input: one value per channel outside [r0 + 1, r1 - 1) and at least c0 - 1 pixels from the edge, random elsewhere
    x = torch.relu(torch.randn(B, Hi, Hi, Ci, generator=g))
    const = torch.relu(torch.randn(Ci, generator=g)) + 0.1
    inner = torch.zeros(Hi, Hi, dtype=torch.bool)
    inner[r0 + 1:r1 - 1, r0 + 1:r1 - 1] = True
    ring = torch.ones(Hi, Hi, dtype=torch.bool)
    ring[c0 - 1:c1 + 1, c0 - 1:c1 + 1] = False
    keep_random = inner | ring
    x = torch.where(keep_random[None, :, :, None], x, const[None, None, None, :]).cuda().bfloat16()
    w = (torch.randn(Co, 3, 3, Ci, generator=g) / (Ci * 9) ** 0.5).cuda().bfloat16()
    bias = torch.randn(Co, generator=g).cuda()
    Hp = (Hi + 1) // 2
    lib = L.load()
    res = []
    for cb_on in (0, 1):
        for pool_only in (0, 1):
            out = torch.full((B, Hi, Hi, Co), 3.0, device="cuda", dtype=torch.bfloat16)
            pool = torch.full((B, Hp, Hp, Co), 5.0, device="cuda", dtype=torch.bfloat16)
            code = torch.full((B, Hp, Hp, Co), 9, device="cuda", dtype=torch.uint8)
            ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
            d = L.ConvDesc(dt, B, Hi, Hi, Ci, Hi, Hi, Co, 3, 3, 1, Ci, Co, 0, 1, 0)
            d.pool_out, d.pool_code, d.pool_only = pool.data_ptr(), code.data_ptr(), pool_only
            d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
            if cb_on:
                d.cb_on = 1
                for i, v in enumerate((r0, r1, r0, r1)):
                    d.cb_rect[i] = v
                for i, v in enumerate((c0, c1, c0, c1)):
                    d.cb_const[i] = v
            L.call("szn_conv2d_fwd", C.byref(d), L.ptr(x), L.ptr(w), L.ptr(bias), None, None, L.ptr(out), L.stream_ptr())
            assert L.last_kernel() == "conv3x3_regw", L.last_kernel()
            frac = d.res.work_fraction
            torch.cuda.synchronize()
            res.append((cb_on, pool_only, out, pool, code, frac))
    dense = res[0]
    assert dense[5] == 1.0
    for cb_on, pool_only, out, pool, code, frac in res[1:]:
        assert torch.equal(pool, dense[3]) and torch.equal(code, dense[4]), (cb_on, pool_only)
        if not pool_only:
            assert torch.equal(out, dense[2]), (cb_on, pool_only)
        if cb_on:
            assert 0.3 < frac < 0.9, frac                 # tiles were actually skipped


@pytest.mark.parametrize("case", [(2, 710, 64, 64, (98, 612, 98, 612), (98, 612, 96, 640)), (1, 300, 64, 64, (50, 210, 40, 222), (50, 210, 32, 224))])
def test_constant_border_hint_of_a_gated_dgrad(case):
    """szn_conv_desc_t.cb_on on szn_conv2d_dgrad (conv1_2's dgrad): the gate is read from one reference pixel where the caller says it is
    constant, stores outside the rectangle the consumer reads are skipped -- din inside that rectangle and the column sums (conv1_1's
    bias gradient) are the same bits as the dense run, and the skipped region really is left alone"""
    B, Hi, Ci, Co, grect, srect = case
    g = torch.Generator().manual_seed(37)
    dt = L.dtype_code(torch.bfloat16)
    dout = torch.randn(B, Hi, Hi, Co, generator=g).cuda().bfloat16()
    gate = torch.relu(torch.randn(B, Hi, Hi, Ci, generator=g))
    const = torch.relu(torch.randn(Ci, generator=g))                    # zeros and positive values: channels gated off and on
    inside = torch.zeros(Hi, Hi, dtype=torch.bool)
    inside[grect[0]:grect[1], grect[2]:grect[3]] = True
    gate = torch.where(inside[None, :, :, None], gate, const[None, None, None, :]).cuda().bfloat16()
    wT = (torch.randn(Ci, 3, 3, Co, generator=g) / (Co * 9) ** 0.5).cuda().bfloat16()
    res = []
    for cb_on in (0, 1):
        din = torch.full((B, Hi, Hi, Ci), 7.0, device="cuda", dtype=torch.bfloat16)
        colsum = torch.zeros(Ci, device="cuda")
        slab = torch.zeros(1024, Ci, device="cuda")
        d = L.ConvDesc(dt, B, Hi, Hi, Ci, Hi, Hi, Co, 3, 3, 1, Ci, Co, Ci, 0, 0)
        d.colsum, d.colsum_slab, d.colsum_slab_rows = colsum.data_ptr(), slab.data_ptr(), 1024
        if cb_on:
            d.cb_on = 1
            for i in range(4):
                d.cb_rect[i], d.cb_const[i] = grect[i], srect[i]
        L.call("szn_conv2d_dgrad", C.byref(d), L.ptr(dout), L.ptr(wT), L.ptr(gate), None, L.ptr(din), L.stream_ptr())
        assert L.last_kernel() == "conv3x3_regw", L.last_kernel()
        rows = d.res.colsum_rows
        torch.cuda.synchronize()
        res.append((din, slab[:rows].clone()))
    (dense, cs0), (hint, cs1) = res
    r0, r1, c0, c1 = srect
    assert torch.equal(hint[:, r0:r1, c0:c1], dense[:, r0:r1, c0:c1])
    assert torch.equal(cs0, cs1)
    assert not (dense == 7.0).all(dim=-1).any()
    untouched = (hint == 7.0).all(dim=-1)                                # pixels the hinted run did not store
    assert untouched.float().mean() > 0.2 and not untouched[:, r0:r1, c0:c1].any()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("geom", [(1, 45, 512, 512), (1, 89, 512, 256), (2, 23, 512, 256)])
def test_splitk_epilogue_with_column_sums(dtype, geom):
    """Few output tiles + a long K range (conv4_x / conv5_x dgrads of a one-image step): the library splits K, and since round 5 the split-K
    epilogue also delivers the column sums of the tensor it stores (splitk_epilogue_cs) -- the bias gradient of the producing layer,
    models.py:117-143 backward -- from the fp32 values.  The tensor equals the one the plain split-K epilogue writes bit for bit; the
    column sums equal those of the unsplit kernel's epilogue to fp32 re-ordering and are bit-reproducible (slab + fixed-order reduce)."""
    B, H, Cin, Cout = geom                          # a dgrad call: "Ci" = channels of dout, "Co" = channels of din
    g = torch.Generator(device="cuda").manual_seed(7 + H)
    dout = (torch.randn(B, H, H, Cin, device="cuda", generator=g) * 0.1).to(dtype)
    wT = (torch.randn(Cout, 3, 3, Cin, device="cuda", generator=g) / (9 * Cin) ** 0.5).to(dtype)
    gate = torch.randn(B, H, H, Cout, device="cuda", generator=g).to(dtype)
    code = L.dtype_code(dtype)
    st = L.stream_ptr()
    ws = torch.empty(16 * B * H * H * Cout * 4, dtype=torch.uint8, device="cuda")

    def run(colsum, workspace, slab_rows=0):
        d = L.ConvDesc(code, B, H, H, Cin, H, H, Cout, 3, 3, 1, Cin, Cout, Cout, 0, 0)
        out = torch.full((B, H, H, Cout), float("nan"), device="cuda", dtype=dtype)
        cs = torch.zeros(Cout, device="cuda")
        slab = torch.zeros(max(slab_rows, 1) * Cout, device="cuda")
        if workspace:
            d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
        if colsum:
            d.colsum = cs.data_ptr()
            if slab_rows:
                d.colsum_slab, d.colsum_slab_rows = slab.data_ptr(), slab_rows
        L.call("szn_conv2d_fwd", C.byref(d), L.ptr(dout), L.ptr(wT), None, L.ptr(gate), None, L.ptr(out), st)
        kern = L.last_kernel()
        rows = d.res.colsum_rows
        if colsum and slab_rows:
            assert float(cs.abs().max()) == 0.0 and rows > 0
            L.call("szn_colsum_reduce_batch", 1, (C.c_void_p * 1)(slab.data_ptr()), (C.c_int * 1)(rows), (C.c_int * 1)(Cout),
                   (C.c_void_p * 1)(cs.data_ptr()), st)
        torch.cuda.synchronize()
        return out, cs, kern

    o_plain, _, k_plain = run(False, True)
    assert k_plain == "splitk_epilogue", k_plain                  # the shape really takes the split-K path
    o_cs, cs_slab, k_cs = run(True, True, slab_rows=1024)
    assert k_cs == "splitk_epilogue_cs", k_cs
    o_cs2, cs_slab2, _ = run(True, True, slab_rows=1024)
    o_at, cs_atomic, k_at = run(True, True)                       # no slab: fp32 atomics on colsum
    assert k_at == "splitk_epilogue_cs", k_at
    o_uns, cs_uns, k_uns = run(True, False, slab_rows=1024)       # no scratch: the unsplit kernel and its own epilogue sums
    assert "splitk" not in k_uns
    assert torch.equal(o_cs, o_plain) and torch.equal(o_at, o_plain) and torch.equal(o_cs2, o_plain)
    assert torch.equal(cs_slab, cs_slab2)                         # bit-reproducible
    scale = float(cs_uns.abs().max())
    assert float((cs_slab - cs_uns).abs().max()) < 2e-5 * scale + 1e-6
    assert float((cs_atomic - cs_uns).abs().max()) < 2e-5 * scale + 1e-6
    # and they are the column sums of the stored tensor (16-bit storage: to its rounding)
    ref = o_plain.float().sum(dim=(0, 1, 2))
    tol = 1e-5 if dtype == torch.float32 else 4e-3
    assert float((cs_slab - ref).abs().max()) < tol * float(o_plain.float().abs().sum(dim=(0, 1, 2)).max())
