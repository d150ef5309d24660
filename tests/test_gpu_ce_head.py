"""GPU: the fused softmax cross-entropy head (szn_fused_ce_head) and the cross-entropy TrainStep of train.py -c 1.

  1. the kernel against the materialised chain szn_bilinear_up_crop_fwd -> szn_ce2d_fwd -> szn_ce2d_bwd -> szn_bilinear_up_crop_bwd
     on the same coarse map: prediction bit-equal, loss / counts / d(coarse), 16-bit outputs, untouched padding, forward-only and
     pred-only calls, bitwise reproducibility;
  2. the cfg-1 step through TrainStep against the CPU oracle (backward given the HIP forward state, tests/helpers_parity.py);
  3. TrainStep(loss="cross_entropy") against the autograd route train.py -c 1 ran before (and its fused_head=False form);
  4. FCN8s + cross entropy against its autograd route;
  5. fp16 with the dynamic loss scale;
  6. the trainer, the CLI with --precision fp16 and validation through softmax_predict;
  7. two data-parallel ranks on one GPU against one process with both images.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import szn_oracle as O  # noqa: E402
from helpers_parity import adopt_forward  # noqa: E402
from zeroshotsemanticsegmentation_amd import _lib as L  # noqa: E402
from zeroshotsemanticsegmentation_amd import engine, models, synth, utils  # noqa: E402

SENT = -7.25          # sentinel of the channels outside [c0, c0 + C)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rel(a, b):
    a = a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)
    b = b.detach().double().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


# ----------------------------------------------------------------------------------------------- 1. kernel vs materialised chain
def _labels(B, H, W, C, seed):
    rs = np.random.RandomState(seed)
    t = rs.randint(0, C, size=(B, H, W)).astype(np.int64)
    r = rs.rand(B, H, W)
    t[r < 0.05] = -1                        # unlabelled
    t[(r >= 0.05) & (r < 0.08)] = -2        # batch padding
    t[(r >= 0.08) & (r < 0.10)] = C + rs.randint(0, 3)     # out of range: ignored
    return t


def _ce_call(S, B, h, w, C, ldc, c0, H, W, crop, coarse, target, weight, sa, want_loss=True, want_pred=True, dtype=None):
    dev = coarse.device
    ws = torch.empty(L.load().szn_fused_ce_head_workspace_bytes(S, B, h, w, C), dtype=torch.uint8, device=dev)
    loss = torch.empty(1, device=dev) if want_loss else None
    stats = torch.empty(B, 2, device=dev) if want_loss else None
    pred = torch.empty(B, H, W, dtype=torch.int64, device=dev) if want_pred else None
    dc = None
    if dtype is not None:
        dc = torch.full((B, h, w, ldc), SENT, device=dev, dtype=dtype)
    L.call("szn_fused_ce_head", S, B, h, w, C, ldc, c0, H, W, crop, L.ptr(coarse), L.ptr(target if want_loss else None),
           L.ptr(weight), sa, L.ptr(loss), L.ptr(stats), L.ptr(pred), L.dtype_code(dtype) if dc is not None else 0, L.ptr(dc),
           L.ptr(ws), L.stream_ptr())
    return loss, stats, pred, dc


CASES = [  # stride, C, B, H, W, ldc - C - c0, c0, weighted, size_average
    (32, 21, 1, 512, 512, 0, 0, False, 0),
    (32, 2, 3, 97, 131, 5, 3, False, 1),
    (32, 59, 3, 97, 131, 0, 2, True, 0),
    (32, 256, 1, 97, 131, 4, 0, True, 1),
    (8, 21, 3, 97, 131, 3, 1, False, 0),
    (8, 2, 1, 97, 131, 0, 0, True, 1),
    (8, 59, 1, 97, 131, 2, 5, False, 1),
    (8, 256, 3, 97, 131, 0, 0, True, 0),
]


@pytest.mark.parametrize("case", CASES)
def test_kernel_vs_materialised_chain(case):
    S, C, B, H, W, extra, c0, weighted, sa = case
    crop = 19 if S == 32 else 31
    h, w = (H + crop + S - 1) // S, (W + crop + S - 1) // S
    ldc = c0 + C + extra
    seed = S * 1000 + C
    coarse = torch.full((B, h, w, ldc), 123.0)
    coarse[..., c0:c0 + C] = torch.from_numpy(synth.uniform(seed, (B, h, w, C), -4, 4))
    coarse = coarse.cuda()
    t = cu(_labels(B, H, W, C, seed + 1))
    wt = cu(np.random.RandomState(seed + 2).uniform(0.2, 2.0, C).astype(np.float32)) if weighted else None
    st = L.stream_ptr()
    # the materialised chain
    score = torch.empty(B, C, H, W, device="cuda")
    L.call("szn_bilinear_up_crop_fwd", S, B, h, w, C, ldc, c0, H, W, crop, L.ptr(coarse), L.ptr(score), st)
    ws = torch.empty(L.load().szn_loss_workspace_bytes(B, H, W), dtype=torch.uint8, device="cuda")
    rloss, rstats = torch.empty(1, device="cuda"), torch.empty(B, 2, device="cuda")
    rpred = torch.empty(B, H, W, dtype=torch.int64, device="cuda")
    L.call("szn_ce2d_fwd", B, C, H, W, L.ptr(score), L.ptr(t), L.ptr(wt), sa, L.ptr(rloss), L.ptr(rstats), L.ptr(rpred), L.ptr(ws), st)
    dscore = torch.empty_like(score)
    L.call("szn_ce2d_bwd", B, C, H, W, L.ptr(score), L.ptr(t), L.ptr(wt), sa, L.ptr(rstats), None, L.ptr(dscore), st)
    rdc = torch.zeros(B, h, w, ldc, device="cuda")
    L.call("szn_bilinear_up_crop_bwd", S, B, h, w, C, ldc, c0, H, W, crop, L.ptr(dscore), L.ptr(rdc), st)
    del score, dscore
    # the fused head
    loss, stats, pred, dc = _ce_call(S, B, h, w, C, ldc, c0, H, W, crop, coarse, t, wt, sa, dtype=torch.float32)
    torch.cuda.synchronize()
    assert torch.equal(pred, rpred)
    assert abs(float(loss) - float(rloss)) <= 1e-6 * abs(float(rloss))
    assert torch.equal(stats[:, 1], rstats[:, 1])                                     # valid-pixel counts: exact
    assert rel(stats[:, 0], rstats[:, 0]) < 1e-6
    ref = rdc[..., c0:c0 + C]
    assert rel(dc[..., c0:c0 + C], ref) <= 1e-5, rel(dc[..., c0:c0 + C], ref)
    assert bool((dc[..., :c0] == SENT).all()) and bool((dc[..., c0 + C:] == SENT).all())
    # 16-bit d(coarse): bf16 = the rounding of the fp32 result; fp16 within one fp16 step of it (the in-kernel conversion and
    # torch's may round a few values differently); padding untouched
    for dt in (torch.bfloat16, torch.float16):
        _, _, _, d16 = _ce_call(S, B, h, w, C, ldc, c0, H, W, crop, coarse, t, wt, sa, want_pred=False, dtype=dt)
        got, want = d16[..., c0:c0 + C], dc[..., c0:c0 + C].to(dt)
        if dt == torch.bfloat16:
            assert torch.equal(got, want)
        else:
            ref32 = dc[..., c0:c0 + C]
            step = torch.clamp(ref32.abs(), min=2.0 ** -14) * 2.0 ** -10          # one fp16 ulp (2^-24 in the subnormal range)
            assert bool(((got.float() - ref32).abs() <= step).all())
        assert bool((d16[..., :c0] == SENT).all()) and bool((d16[..., c0 + C:] == SENT).all())
    # forward-only and pred-only calls
    l2, s2, p2, _ = _ce_call(S, B, h, w, C, ldc, c0, H, W, crop, coarse, t, wt, sa)
    _, _, p3, _ = _ce_call(S, B, h, w, C, ldc, c0, H, W, crop, coarse, t, wt, sa, want_loss=False)
    # a second full call: bitwise equal
    l4, s4, p4, d4 = _ce_call(S, B, h, w, C, ldc, c0, H, W, crop, coarse, t, wt, sa, dtype=torch.float32)
    torch.cuda.synchronize()
    assert torch.equal(p2, pred) and torch.equal(p3, pred) and torch.equal(l2, loss) and torch.equal(s2, stats)
    assert torch.equal(l4, loss) and torch.equal(s4, stats) and torch.equal(p4, pred) and torch.equal(d4, dc)


# ----------------------------------------------------------------------------------------------- 2. cfg-1 step vs the oracle
def _oracle_params(m):
    return {k: v.detach().cpu().numpy() for k, v in m.named_parameters() if k.split(".")[0] != "upscore"}


def _probe_idx(n, cnt=64):
    return (np.arange(cnt, dtype=np.int64) * 2654435761 % n).astype(np.int64)


@pytest.mark.parametrize("variant", ["sgd", "sgd_bf16x3", "adam"])
def test_cfg1_train_step_vs_oracle(variant):
    """configs[0] through TrainStep: 21 classes, 256x256, B = 1, CE sum, SGD 1e-10 / .99 / wd 5e-4, biases at 2x lr without wd"""
    Cn, H = 21, 256
    m = models.FCN32s(Cn)
    m.load_synthetic(1337, device=torch.device("cuda"))
    m.eval()
    x = synth.make_images(1, H, H, seed=41)
    target = synth.make_labels(1, H, H, Cn, seed=42)
    om = O.FCN32sOracle(_oracle_params(m), Cn)
    adam = variant == "adam"
    lr = 1e-6 if adam else 1e-10
    ts = engine.TrainStep(m, None, loss="cross_entropy", optimizer="adam" if adam else "sgd", lr=lr, momentum=0.99,
                          weight_decay=0.0005, precision="bf16x3" if variant == "sgd_bf16x3" else torch.float32)
    ts.keep_ctx = True
    gtol = 1e-3 if variant == "sgd_bf16x3" else 1e-4
    oopt = O.Adam(lr) if adam else O.SGD(lr, 0.99)
    try:
        for it in range(2 if variant == "sgd" else 1):
            loss, pred = ts.step(cu(x), cu(target))
            torch.cuda.synchronize()
            ctx = ts.last_ctx
            of = om.forward(x, "fcn")
            oloss, _, _ = O.cross_entropy2d(of, target, size_average=False, want_grad=False)
            assert abs(float(loss) - float(oloss)) < 1e-4 * abs(float(oloss)), (float(loss), float(oloss))
            # the oracle's cross entropy on the HIP score: argmax and the gradient the backward starts from
            sn = m._engine.upscore(ctx).cpu().numpy()
            _, ods, opred = O.cross_entropy2d(sn, target, size_average=False)
            assert np.array_equal(pred.cpu().numpy(), opred)
            assert adopt_forward(om, ctx, x, None, Cn) == 0.0
            og = om.backward(df=ods)
            og = {k: v for k, v in og.items() if k.split(".")[0] in O.WEIGHT_GROUP}
            for k, r in og.items():
                name, kind = k.split(".")
                e = rel(getattr(getattr(m, name), kind).grad, r)
                assert e < (10 if kind == "bias" else 1) * gtol, (k, it, e)
            if adam:
                oopt.step(om.p, og, lambda k: lr * (2 if k.endswith(".bias") else 1))
            else:
                oopt.step(om.p, og, lambda k: lr * (2 if k.endswith(".bias") else 1), lambda k: 0.0 if k.endswith(".bias") else 0.0005)
            for key in ("conv1_1.weight", "conv3_2.weight", "fc6.weight", "fc7.bias", "score_fr.weight", "score_fr.bias"):
                name, kind = key.split(".")
                p = getattr(getattr(m, name), kind).detach()
                idx = _probe_idx(p.numel())
                got = p.flatten()[cu(idx)].cpu().numpy().astype(np.float64)
                want = om.p[key].reshape(-1)[idx].astype(np.float64)
                ulp = np.abs(want).max() * 2.0 ** -23
                if adam:        # Adam's first step is lr * g / (|g| + eps): compare where the gradient is well above eps
                    g = np.abs(og[key].reshape(-1)[idx])
                    big = g > 1e-3 * np.abs(og[key]).max()
                    assert big.any() and np.abs(got - want)[big].max() <= 2 * ulp + 1e-3 * lr, (key, it)
                else:
                    assert np.abs(got - want).max() <= 2 * ulp, (key, it)
            om.p.update({k: np.ascontiguousarray(v) for k, v in _oracle_params(m).items()})
    finally:
        ts.last_ctx = None


# ----------------------------------------------------------------------------------------------- 3. TrainStep vs the autograd route
def _sgd_step(m, fused_head=True):
    return engine.TrainStep(m, None, loss="cross_entropy", optimizer="sgd", lr=1e-10, momentum=0.99, weight_decay=0.0005,
                            precision=torch.float32, fused_head=fused_head)


def _grad_rel(ma, mb, names):
    out = {}
    for n in names:
        for kind in ("weight", "bias"):
            out["%s.%s" % (n, kind)] = rel(getattr(getattr(mb, n), kind).grad, getattr(getattr(ma, n), kind).grad)
    return out


def test_train_step_equals_autograd_route():
    from zeroshotsemanticsegmentation_amd.configs import configurations
    from zeroshotsemanticsegmentation_amd.train import make_fcn_optimizer
    Cn, H, B = 21, 256, 2
    dev = torch.device("cuda")
    x = cu(synth.make_images(B, H, H, seed=43))
    t = cu(synth.make_labels(B, H, H, Cn, seed=44))
    ma = models.FCN32s(Cn).load_synthetic(1337, device=dev).eval()
    opt = make_fcn_optimizer(ma, configurations[1])
    mb = models.FCN32s(Cn).load_synthetic(1337, device=dev).eval()
    mc = models.FCN32s(Cn).load_synthetic(1337, device=dev).eval()
    tb, tc = _sgd_step(mb), _sgd_step(mc, fused_head=False)
    for it in range(2):
        score = ma(x, mode="fcn")
        loss = utils.cross_entropy2d(score, t, size_average=False)
        apred = utils.channel_argmax(score)
        opt.zero_grad()
        loss.backward()
        opt.step()
        lb, pb = tb.step(x, t)
        lc, pc = tc.step(x, t)
        torch.cuda.synchronize()
        assert torch.equal(pb, apred) and torch.equal(pc, apred)
        assert abs(float(lb) - float(loss)) < 1e-6 * abs(float(loss)) and abs(float(lc) - float(loss)) < 1e-6 * abs(float(loss))
        for mm in (mb, mc):
            # gradients on the same forward state (step 1; afterwards the weights differ in the last bit here and there, and
            # ReLU / pooling flips move whole gradient elements: tests/helpers_parity.py)
            if it == 0:
                for k, e in _grad_rel(ma, mm, models._OPT_LAYERS).items():
                    assert e < 1e-4, (k, it, e)
            for (na, pa), (nb, pb_) in zip(ma.named_parameters(), mm.named_parameters()):
                assert na == nb
                if na.split(".")[0] in models._OPT_LAYERS:
                    # step 2 starts from weights that differ in the last bit here and there (step 1's updates round
                    # differently): its ReLU / pooling flips widen the tolerance
                    assert rel(pb_, pa) < (1e-5 if it == 0 else 2e-4), (na, it)


# ----------------------------------------------------------------------------------------------- 4. FCN8s
def test_fcn8s_train_step_vs_autograd():
    Cn, H, B = 21, 256, 1
    dev = torch.device("cuda")
    x = cu(synth.make_images(B, H, H, seed=45))
    t = cu(synth.make_labels(B, H, H, Cn, seed=46))
    ma = models.FCN8s(Cn).load_synthetic(1337, device=dev).eval()
    mb = models.FCN8s(Cn).load_synthetic(1337, device=dev).eval()
    score = ma(x, mode="fcn")
    loss = utils.cross_entropy2d(score, t, size_average=False)
    loss.backward()
    ts = _sgd_step(mb)
    lb, pb = ts.step(x, t)
    torch.cuda.synchronize()
    assert torch.equal(pb, utils.channel_argmax(score))
    assert abs(float(lb) - float(loss)) < 1e-6 * abs(float(loss))
    for k, e in _grad_rel(ma, mb, models.opt_layers(mb)).items():
        assert e < 1e-5, (k, e)
    # inference through softmax_predict: same prediction, same loss
    with torch.no_grad():
        l2, p2 = ma.softmax_predict(x, t)
        s2 = ma(x, mode="fcn")
    assert torch.equal(p2, utils.channel_argmax(s2))
    ref = float(utils.cross_entropy2d(s2, t, size_average=False))
    assert abs(float(l2) - ref) < 1e-6 * abs(ref)


# ----------------------------------------------------------------------------------------------- 5. fp16
def _cos(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a @ b) / (a.norm() * b.norm()))


def test_fp16_ce_steps():
    Cn, H, B = 21, 256, 2
    dev = torch.device("cuda")
    x = cu(synth.make_images(B, H, H, seed=47))
    t = cu(synth.make_labels(B, H, H, Cn, seed=48))
    m = models.FCN32s(Cn).load_synthetic(1337, device=dev).eval()
    snap = {k: v.detach().clone() for k, v in m.state_dict().items()}
    ts = engine.TrainStep(m, None, loss="cross_entropy", optimizer="sgd", lr=1e-10, precision=torch.float16)
    assert ts.dynamic
    losses, first = [], None
    for i in range(6):
        scale = ts.loss_scale
        applied = ts.applied_steps
        loss, _ = ts.step(x, t)
        losses.append(float(loss))
        if first is None and ts.applied_steps == applied + 1:
            first = (i, {n: getattr(m, n).weight.grad.detach().float() / scale for n in ("score_fr", "fc7")})
        if first is None:       # the next step starts from these (unchanged) weights
            snap = {k: v.detach().clone() for k, v in m.state_dict().items()}
    assert all(np.isfinite(losses)), losses
    assert ts.applied_steps >= 5, (ts.applied_steps, losses)
    assert first is not None
    m32 = models.FCN32s(Cn).to(dev).eval()
    m32.load_state_dict(snap)
    m32._engine.mark_dirty()
    ts32 = engine.TrainStep(m32, None, loss="cross_entropy", optimizer="sgd", lr=1e-10, precision=torch.float32)
    ts32.step(x, t)
    torch.cuda.synchronize()
    for n, g16 in first[1].items():
        c = _cos(g16, getattr(m32, n).weight.grad)
        assert c >= 0.99, (n, first[0], c)


# ----------------------------------------------------------------------------------------------- 6. trainer and CLI
def test_trainer_and_cli_fp16(tmp_path):
    import glob
    from zeroshotsemanticsegmentation_amd import train, trainer_fcn
    from zeroshotsemanticsegmentation_amd.configs import configurations
    from zeroshotsemanticsegmentation_amd.synthetic_dataset import SyntheticSegmentation
    d = str(tmp_path)
    train.main(['-c', '1', '--precision', 'fp16', '--synthetic', '2', '256', '256', '-ve', '1', '-dir', d, '-n', 'cfg1h',
                '--workers', '0'])
    log = glob.glob(os.path.join(d, 'logs', 'cfg1h_CFG_1_*'))[0]
    rows = open(os.path.join(log, 'train_log.csv')).read().strip().split('\n')
    losses = [float(r.split(',')[2]) for r in rows[1:]]
    assert len(losses) == 2 and all(np.isfinite(losses)), losses
    # the trainer's step and its validation route
    Cn, H = 21, 96
    m = models.FCN32s(Cn).load_synthetic(1337, device=torch.device("cuda"))
    ds = SyntheticSegmentation(split="val", n_images=2, size=(H, H + 16), n_class=Cn, embed_dim=0, seed=5)
    loader = torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False)
    opt = train.make_fcn_optimizer(m, configurations[1])
    tr = trainer_fcn.Trainer(cuda=True, model=m, optimizer=opt, train_loader=loader, val_loader=loader, log_dir=d,
                             dataset="pascal", max_epoch=1, tb_writer=None, pixel_embeddings=0, loss_func="cross_entropy")
    assert isinstance(tr._fast_step(), engine.TrainStep) and tr._step.ce
    m.eval()
    hists, sums = [], []
    for verbose in (False, True):
        tr.verbose_val = verbose
        hist = torch.zeros(3, Cn, Cn, dtype=torch.int64, device="cuda")
        s = 0.0
        with torch.no_grad():
            for data, target in loader:
                score, loss, pred, tgt = tr._predict_device(data, target, False)
                assert (score is None) != verbose
                s += float(loss)
                utils.confusion_hist_device(tgt, pred, Cn, None, hist)
        hists.append(hist.cpu())
        sums.append(s)
    assert torch.equal(hists[0], hists[1])
    assert abs(sums[0] - sums[1]) <= 1e-6 * abs(sums[1])


# ----------------------------------------------------------------------------------------------- 7. data parallel
DP_C, DP_H = 21, 64          # the geometry of tests/test_gpu_ddp_single_gpu.py: B = 1 and B = 2 run the same kernels


def _dp_data():
    return synth.make_images(2, DP_H, DP_H, seed=63), synth.make_labels(2, DP_H, DP_H, DP_C, seed=64, block=16)


def _dp_worker(rank, world, port, q):
    try:
        import torch.distributed as dist
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        x, t = _dp_data()
        dev = torch.device("cuda", 0)
        m = models.FCN32s(DP_C).load_synthetic(1337, device=dev).eval()
        ts = engine.TrainStep(m, None, loss="cross_entropy", optimizer="sgd", lr=1e-10, precision=torch.float32, bucket_mb=25)
        assert ts.world == 2
        try:
            engine.TrainStep(m, None, loss="cross_entropy", size_average=True, precision=torch.float32)
            raise AssertionError("size_average=True accepted with two ranks")
        except L.SznError:
            pass
        ts.step(torch.from_numpy(x[rank:rank + 1]).to(dev), torch.from_numpy(t[rank:rank + 1]).to(dev))
        torch.cuda.synchronize()
        out = {"rank": rank}
        if rank == 0:
            out["gw"] = (ts.flat_gw * 0.5).cpu().numpy()          # what the optimizer consumed: sum x 1/world
            out["gb"] = (ts.flat_gb * 0.5).cpu().numpy()
        q.put(out)
        dist.barrier()
        dist.destroy_process_group()
    except Exception as ex:
        import traceback
        q.put({"rank": rank, "error": "%r\n%s" % (ex, traceback.format_exc())})


def test_two_ranks_mean_gradient():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31700 + os.getpid() % 2000
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    for _ in procs:
        o = q.get(timeout=600)
        assert "error" not in o, o.get("error")
        res[o["rank"]] = o
    for p in procs:
        p.join(120)
    x, t = _dp_data()
    m = models.FCN32s(DP_C).load_synthetic(1337, device=torch.device("cuda", 0)).eval()
    ts = engine.TrainStep(m, None, loss="cross_entropy", optimizer="sgd", lr=1e-10, precision=torch.float32)
    ts.step(cu(x), cu(t))
    torch.cuda.synchronize()
    gw, gb = 0.5 * ts.flat_gw.cpu().numpy(), 0.5 * ts.flat_gb.cpu().numpy()
    assert np.abs(res[0]["gw"] - gw).max() < 1e-5 * np.abs(gw).max()
    assert np.abs(res[0]["gb"] - gb).max() < 1e-5 * np.abs(gb).max()
