"""GPU: gradient-norm clipping and the gradient log on engine.TrainStep(clip=) and through the Trainer -- max_norm = inf changes
nothing, a finite max_norm is the existing optimizer entry with the gradient scale times the coefficient, the launches sit where they
must, the dynamic loss scale's skip is raised by szn_clip_coef, the statistics are read from the wire image of a forced one-rank
exchange, the refusals, and train.py --clip-grad-norm.  B = 2, 64 x 64, K = 21, E = 20 (tests/test_gpu_ema_engine.py's shapes)."""
import glob
import math
import os
import re
import shutil
import sys
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers_clip as R  # noqa: E402
from zeroshotsemanticsegmentation_amd import _lib as L  # noqa: E402
from zeroshotsemanticsegmentation_amd import engine, models, synth, train, trainer_fcn  # noqa: E402
from zeroshotsemanticsegmentation_amd.configs import configurations  # noqa: E402
from zeroshotsemanticsegmentation_amd.synthetic_dataset import SyntheticSegmentation  # noqa: E402

E, K, B, H, W = 20, 21, 2, 64, 64
EMB = synth.make_embeddings(K, E)
ARCH = {"fcn32s": models.FCN32s, "fcn8s": models.FCN8s}
CASES = [("fcn32s", torch.float32, "adam"), ("fcn32s", torch.bfloat16, "adam"), ("fcn32s", torch.float16, "adam"),
         ("fcn32s", torch.bfloat16, "sgd"), ("fcn8s", torch.bfloat16, "adam")]
IDS = ["%s-%s-%s" % (a, str(p).split(".")[1], o) for a, p, o in CASES]
INF = float("inf")


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def batch():
    return cu(synth.make_images(B, H, W, seed=71)), cu(synth.make_labels(B, H, W, K, seed=72, block=8))


def fresh(arch="fcn32s", precision=torch.float32, optimizer="adam", **kw):
    m = ARCH[arch](E).load_synthetic(1337, device=torch.device("cuda")).eval()
    lr = 1e-4 if optimizer == "adam" else 1e-3       # learning rates at which a step moves the weights (and their 16-bit image) visibly
    return engine.TrainStep(m, EMB, optimizer=optimizer, lr=lr, precision=precision, **kw)


def buffers(ts):
    out = [ts.flat_w, ts.flat_b] + list(ts.state["w"]) + list(ts.state["b"])
    return out + ([ts.flat_w_lp] if ts.flat_w_lp is not None else [])


def view_bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return len(a) == len(b) and all(torch.equal(view_bits(x), view_bits(y)) for x, y in zip(a, b))


def norm64(ts, gw, gb, factor):
    """float64 norms of the gradient buffers: (global, {segment: norm}), times `factor`"""
    seg = {}
    for name, off, g in [(n + ".weight", ts.woff[n], gw) for n in ts.layers] + [(n + ".bias", ts.boff[n], gb) for n in ts.layers]:
        seg[name] = math.sqrt(float(g[off[0]:off[0] + off[1]].double().pow(2).sum())) * factor
    return math.sqrt(sum(v * v for v in seg.values())), seg


@pytest.mark.parametrize("arch,precision,optimizer", CASES, ids=IDS)
def test_max_norm_inf_changes_nothing(arch, precision, optimizer):
    x, t = batch()
    ts, twin = fresh(arch, precision, optimizer, clip=dict(max_norm=INF)), fresh(arch, precision, optimizer)
    assert twin.grad_stats is None and twin.clip_state is None and not ts.fused_adam
    assert ts.grad_segments == [n + ".weight" for n in ts.layers] + [n + ".bias" for n in ts.layers]
    assert ts.grad_stats.shape == (2 * len(ts.layers), 2) and ts.grad_stats.dtype == torch.float64 and ts.clip_state.shape == (4,)
    for step in range(1, 5):
        (la, pa), (lb, pb) = ts.step(x, t), twin.step(x, t)
        assert float(la) == float(lb) and np.isfinite(float(la)) and torch.equal(pa, pb)
        assert same_bits(buffers(ts), buffers(twin)), step                   # weights, biases, moments, the 16-bit image
        r = ts.grad_norms()
        assert r["coef"] == 1.0 and r["clipped"] == 0 and r["seen"] == step == ts.applied_steps
        assert 0 < r["norm"] < INF and all(0 <= v < INF for v in r["norms"].values())
        assert abs(math.sqrt(sum(v * v for v in r["norms"].values())) - r["norm"]) <= 1e-6 * r["norm"]


@pytest.mark.parametrize("arch,precision,optimizer", CASES[:4], ids=IDS[:4])
def test_a_finite_max_norm_is_the_existing_entry_with_the_scaled_gradient(arch, precision, optimizer):
    x, t = batch()
    twin = fresh(arch, precision, optimizer, keep_grads=True, fused_adam=False)
    init = [b.clone() for b in buffers(twin)]
    S = twin.loss_scale
    twin.step(x, t)                                                          # its gradient buffers now hold the step's gradients
    factor = twin.grad_factor() / (S if twin.dynamic else 1.0)
    want_norm, want_seg = norm64(twin, twin.flat_gw, twin.flat_gb, factor)
    ts = fresh(arch, precision, optimizer, clip=dict(max_norm=0.5 * want_norm))
    assert same_bits(buffers(ts), init)
    ts.step(x, t)
    r = ts.grad_norms()
    coef = float(ts.clip_state[0])
    want_coef, _, _ = R.clip_ref(ts.grad_stats[:, 1].cpu().numpy(), 0.5 * want_norm, twin.grad_factor(), S if twin.dynamic else 1.0)
    assert coef in R.f32_neighbours(want_coef) and 0.0 < coef <= 0.5
    assert abs(r["norm"] - want_norm) <= 1e-6 * want_norm and r["clipped"] == 1 and r["seen"] == 1
    for n, v in want_seg.items():
        assert abs(r["norms"][n] - v) <= 1e-6 * v, n
    o, cnt = twin.woff["score_fr"]
    want_sum = float(twin.flat_gw[o:o + cnt].double().sum()) * factor
    scale = float(twin.flat_gw[o:o + cnt].double().abs().sum()) * factor
    assert abs(r["sums"]["score_fr.weight"] - want_sum) <= 1e-9 * scale
    # the twin's initial state through the existing entries with grad_scale = fl32(grad_scale * coef)
    eff = float(np.float32(twin.grad_factor()) * np.float32(coef))
    it = iter(init)
    w, b = next(it), next(it)
    sw = [next(it) for _ in twin.state["w"]]
    sb = [next(it) for _ in twin.state["b"]]
    lp = next(it) if twin.flat_w_lp is not None else None
    dyn = torch.tensor([S, 0.0, 0.0, 0.0], device="cuda") if twin.dynamic else None
    st = L.stream_ptr()
    for p, g, state, lr, wd, img in ((w, twin.flat_gw, sw, twin.lr, twin.wd if optimizer == "sgd" else twin.adam_wd, lp),
                                     (b, twin.flat_gb, sb, twin.bias_lr, twin.bias_wd, None)):
        n, ip, ic = p.numel(), L.ptr(img), (L.dtype_code(img.dtype) if img is not None else 0)
        if optimizer == "adam":
            hp = (float(lr), float(twin.betas[0]), float(twin.betas[1]), float(twin.eps), float(wd))
            if dyn is not None:
                L.call("szn_adam_step_scaled", n, L.ptr(p), L.ptr(g), L.ptr(state[0]), L.ptr(state[1]), *hp, L.ptr(dyn), eff, ip, ic, st)
            else:
                L.call("szn_adam_step", n, L.ptr(p), L.ptr(g), L.ptr(state[0]), L.ptr(state[1]), *hp, 1, eff, ip, ic, st)
        else:
            L.call("szn_sgd_momentum_step", n, L.ptr(p), L.ptr(g), L.ptr(state[0]), float(lr), float(twin.momentum), float(wd), 1, eff, ip,
                   ic, st)
    assert same_bits(buffers(ts), init)                                      # (init was updated in place)
    assert not same_bits(buffers(ts)[:1], buffers(twin)[:1])                 # and the clipped step is not the plain step


def test_launch_order(monkeypatch):
    x, t = batch()
    names = []
    real = L.call

    def call(name, *a):
        names.append(name)
        return real(name, *a)

    def record(s):
        del names[:]
        with monkeypatch.context() as mp:
            mp.setattr(L, "call", call)
            s.step(x, t)
        return list(names)
    opt_re = re.compile(r"szn_(adam|sgd_momentum)_step")
    for kw in (dict(precision=torch.float16), dict(precision=torch.bfloat16), dict(precision=torch.float32),
               dict(precision=torch.bfloat16, optimizer="sgd"), dict(precision=torch.float16, ema=dict(decay=0.9, warmup=False))):
        seq = record(fresh(clip=dict(max_norm=1.0), **kw))
        i = seq.index("szn_grad_stats")
        opt = "szn_adam_step_clipped" if kw.get("optimizer", "adam") == "adam" else "szn_sgd_momentum_step_clipped"
        tail = ["szn_grad_stats", "szn_grad_stats", "szn_clip_coef", opt, opt]
        tail += ["szn_ema_step", "szn_ema_step"] if "ema" in kw else []
        tail += ["szn_loss_scale_update"] if kw["precision"] == torch.float16 else []
        assert seq[i:i + len(tail)] == tail, (kw, seq[i:])
        assert "szn_grad_check_finite" not in seq and "szn_conv2d_wgrad_adam" not in seq
        assert [n for n in seq if opt_re.match(n)] == [opt, opt] and seq.count("szn_grad_stats") == 2 and seq.count("szn_clip_coef") == 1
        assert not any(opt_re.match(n) for n in seq[:i])                     # no update in front of the statistics
        kw.pop("ema", None)
        off, plain = record(fresh(clip=None, **kw)), record(fresh(**kw))
        assert off == plain and not {"szn_grad_stats", "szn_clip_coef", opt} & set(plain)
    assert "szn_conv2d_wgrad_adam" in record(fresh(precision=torch.bfloat16))          # the epilogue the clipped step switched off


def test_overflowed_steps_are_skipped_on_the_device_and_not_counted():
    """the far-too-large loss scale of test_overflowed_steps_skip_the_average: szn_clip_coef raises found_inf, the optimizer entries skip,
    the scale halves until a step applies"""
    x, t = batch()
    ts = fresh(precision=torch.float16, loss_scale=2.0 ** 40, clip=dict(max_norm=INF))
    assert ts.dynamic
    w0, b0 = ts.flat_w.clone(), ts.flat_b.clone()
    skipped = 0
    for _ in range(60):
        ts.step(x, t)
        if ts.applied_steps:
            break
        skipped += 1
        assert torch.equal(ts.flat_w, w0) and torch.equal(ts.flat_b, b0)
        assert ts.loss_scale == 2.0 ** (40 - skipped)                        # the scale halves
        c = ts.clip_state.cpu().tolist()
        assert c[0] == 1.0 and not math.isfinite(c[1]) and c[2:] == [0.0, 0.0]
    assert skipped >= 1 and ts.applied_steps == 1 and not torch.equal(ts.flat_w, w0)
    r = ts.grad_norms()
    assert (r["coef"], r["clipped"], r["seen"]) == (1.0, 0, 1) and 0 < r["norm"] < INF
    assert float(ts.clip_scale) == 2.0 ** (40 - skipped) == ts.loss_scale    # the scale the applied step's gradients carried
    ts.step(x, t)
    assert ts.applied_steps == 2 and ts.grad_norms()["seen"] == 2           # and training goes on


def test_forced_exchange_wires_and_the_sharded_refusal(tmp_path, monkeypatch):
    import torch.distributed as dist
    x, t = batch()
    dist.init_process_group("gloo", store=dist.FileStore(str(tmp_path / "store"), 1), rank=0, world_size=1)
    try:
        for wire in (torch.float32, torch.bfloat16):
            kw = dict(precision=torch.bfloat16, force_comm=True, grad_comm_dtype=wire, keep_grads=False, direct_wire=True)
            probe = fresh(clip=dict(max_norm=INF), **kw)
            assert probe.buckets.active and probe.buckets.direct == (wire == torch.bfloat16)
            init = [b.clone() for b in buffers(probe)]
            probe.step(x, t)
            nw = probe.flat_gw.numel()
            gw = probe.buckets.stage[:nw] if probe.buckets.direct else probe.flat_gw      # the buffer the optimizer reads
            want_norm, want_seg = norm64(probe, gw, probe.flat_gb, 1.0)
            r = probe.grad_norms()
            assert abs(r["norm"] - want_norm) <= 1e-6 * want_norm            # the statistics were read from the wire image
            for n, v in want_seg.items():
                assert abs(r["norms"][n] - v) <= 1e-6 * v, n
            ts = fresh(clip=dict(max_norm=0.5 * want_norm), **kw)
            ts.step(x, t)
            gw2 = ts.buckets.stage[:nw] if ts.buckets.direct else ts.flat_gw
            assert torch.equal(view_bits(gw2), view_bits(gw))
            coef = float(ts.clip_state[0])
            assert 0.0 < coef <= 0.5 and ts.grad_norms()["clipped"] == 1
            w, b, m1, m2, bm1, bm2, lp = init
            st, hp = L.stream_ptr(), (float(ts.betas[0]), float(ts.betas[1]), float(ts.eps), 0.0)
            if ts.buckets.direct:
                L.call("szn_adam_step_g16", nw, L.ptr(w), L.ptr(gw), L.SZN_BF16, L.ptr(m1), L.ptr(m2), float(ts.lr), *hp, 1, coef, L.ptr(lp),
                       L.SZN_BF16, st)
            else:
                L.call("szn_adam_step", nw, L.ptr(w), L.ptr(gw), L.ptr(m1), L.ptr(m2), float(ts.lr), *hp, 1, coef, L.ptr(lp), L.SZN_BF16, st)
            L.call("szn_adam_step", b.numel(), L.ptr(b), L.ptr(ts.flat_gb), L.ptr(bm1), L.ptr(bm2), float(ts.bias_lr), *hp, 1, coef, None, 0,
                   st)
            assert same_bits(buffers(ts), init)
        monkeypatch.setenv("SZN_SHARDED_OPT", "1")
        with pytest.raises(ValueError) as e:
            fresh(force_comm=True, clip=dict(max_norm=1.0))
        assert "sharded" in str(e.value)
    finally:
        dist.destroy_process_group()


def test_bad_max_norm_is_refused_before_anything_is_built():
    m = models.FCN32s(E).load_synthetic(1337, device=torch.device("cuda")).eval()
    for bad in (dict(max_norm=0.0), dict(max_norm=-1.0), dict(max_norm=float("nan")), dict(), 1.0):
        with pytest.raises(ValueError):
            engine.TrainStep(m, EMB, precision=torch.float32, clip=bad)
    with pytest.raises(L.SznError):
        fresh().grad_norms()


# ---- Trainer and train.py -----------------------------------------------------------------------------------------------------
COMMON = ['-c', '4', '--synthetic', '2', '64', '64', '--workers', '0', '-ve', '1']


def run_dir(d, name):
    logs = glob.glob(os.path.join(d, 'logs', name + '_CFG_*'))
    assert len(logs) == 1, logs
    return logs[0]


def test_train_py_writes_the_gradient_log(capsys):
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    d = tempfile.mkdtemp(prefix="szn_clip_", dir=base)
    try:
        train.main(COMMON + ['-dir', d, '-n', 'clip', '--clip-grad-norm', '1e-3'])
        out = capsys.readouterr().out
        train.main(COMMON + ['-dir', d, '-n', 'plain'])
        plain_out = capsys.readouterr().out
        log = run_dir(d, 'clip')
        rows = [r.split(',') for r in open(os.path.join(log, 'grad_log.csv')).read().strip().split('\n')]
        layers = models.opt_layers(models.FCN32s(20))
        assert rows[0] == ['epoch', 'iteration', 'grad_norm', 'clip_coef', 'clipped_steps'] + [n + ".weight" for n in layers] + \
            [n + ".bias" for n in layers]
        assert [(int(r[0]), int(r[1])) for r in rows[1:]] == [(0, 0), (0, 1)]
        for r in rows[1:]:
            vals = [float(v) for v in r[2:]]
            assert len(r) == len(rows[0]) and all(math.isfinite(v) and v >= 0 for v in vals) and 0 < vals[1] <= 1.0
            assert abs(math.sqrt(sum(v * v for v in vals[3:])) - vals[0]) <= 1e-5 * vals[0]
        assert int(rows[-1][4]) == sum(float(r[3]) < 1.0 for r in rows[1:])
        sums = re.findall(r"score_fr grad sum\s+(\S+) \|", out)
        assert len(sums) == 2 and all(math.isfinite(float(s)) for s in sums)           # a number stands in the column
        plain_sums = re.findall(r"score_fr grad sum\s+(\S+) \|", plain_out)
        assert plain_sums == ['nan', 'nan'] and not os.path.exists(os.path.join(run_dir(d, 'plain'), 'grad_log.csv'))
        assert sorted(os.listdir(run_dir(d, 'plain'))) == sorted(set(os.listdir(log)) - {'grad_log.csv'})
    finally:
        shutil.rmtree(d, ignore_errors=True)


def _trainer(tmp, **kw):
    cfg = configurations[4]
    m = models.FCN32s(20).load_synthetic(1337).cuda()
    ds = SyntheticSegmentation(split="val", n_images=1, size=(64, 64), n_class=21, embed_dim=20, seed=1337)
    loader = torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False)
    return trainer_fcn.Trainer(cuda=True, model=m, optimizer=train.make_fcn_optimizer(m, cfg), train_loader=loader, val_loader=loader,
                               log_dir=str(tmp), dataset="pascal", max_epoch=1, tb_writer=None, pixel_embeddings=20, loss_func="cos", **kw)


def test_trainer_keywords_and_refusal_off_the_fused_step(tmp_path):
    for kw in (dict(clip_grad_norm=1.0), dict(grad_stats=True)):
        with pytest.raises(L.SznError) as e:
            _trainer(tmp_path, fused_step=False, **kw)
        assert str(e.value) == trainer_fcn.clip_refused(True, False)
    with pytest.raises(ValueError):
        _trainer(tmp_path, clip_grad_norm=0.0)
    assert _trainer(tmp_path, grad_stats=True).clip == dict(max_norm=INF)
    assert _trainer(tmp_path, clip_grad_norm=2.0, grad_stats=True).clip == dict(max_norm=2.0)
    t = _trainer(tmp_path)
    assert t.clip is None and t._fast_step().clip_state is None
    assert _trainer(tmp_path, clip_grad_norm=2.0)._fast_step()._clip == 2.0
