"""GPU: averaged weights on engine.TrainStep(ema=) -- the average never feeds back into training, follows the float64 recurrence
(tests/helpers_ema.py, evaluated in float64 on the device), is skipped on the device with the steps the dynamic loss scale skips, and
averaged_weights() is an exact exchange.  B = 2, 64 x 64, K = 21, E = 20; fp32, bf16 (fc6's Adam update in its weight-gradient
kernel) and fp16 with the dynamic loss scale, Adam and SGD, FCN32s and one FCN8s case."""
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
from zeroshotsemanticsegmentation_amd import engine, models, synth  # noqa: E402

E, K, B, H, W = 20, 21, 2, 64, 64
EMB = synth.make_embeddings(K, E)
ARCH = {"fcn32s": models.FCN32s, "fcn8s": models.FCN8s}
CASES = [("fcn32s", torch.float32, "adam"), ("fcn32s", torch.bfloat16, "adam"), ("fcn32s", torch.float16, "adam"),
         ("fcn32s", torch.bfloat16, "sgd"), ("fcn32s", torch.float16, "sgd"), ("fcn8s", torch.bfloat16, "adam")]
IDS = ["%s-%s-%s" % (a, str(p).split(".")[1], o) for a, p, o in CASES]


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def batch():
    return cu(synth.make_images(B, H, W, seed=71)), cu(synth.make_labels(B, H, W, K, seed=72, block=8))


def fresh(arch="fcn32s", precision=torch.float32, optimizer="adam", **kw):
    m = ARCH[arch](E).load_synthetic(1337, device=torch.device("cuda")).eval()
    # learning rates at which a few steps move the weights (and their 16-bit image) visibly
    lr = 1e-4 if optimizer == "adam" else 1e-3
    return engine.TrainStep(m, EMB, optimizer=optimizer, lr=lr, precision=precision, **kw)


def buffers(ts):
    out = [ts.flat_w, ts.flat_b] + list(ts.state["w"]) + list(ts.state["b"])
    return out + ([ts.flat_w_lp] if ts.flat_w_lp is not None else [])


def same_bits(a, b):
    return all(torch.equal(x.view(torch.int16 if x.element_size() == 2 else torch.int32),
                           y.view(torch.int16 if y.element_size() == 2 else torch.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("every", [1, 2])
@pytest.mark.parametrize("arch,precision,optimizer", CASES, ids=IDS)
def test_average_follows_the_recurrence_and_never_feeds_back(arch, precision, optimizer, every):
    x, t = batch()
    cfg = dict(decay=0.9, every=every)
    ts, twin = fresh(arch, precision, optimizer, ema=cfg), fresh(arch, precision, optimizer)
    assert twin.ema_w is None and ts.ema_w.dtype == torch.float32 and ts.ema_w.data_ptr() != ts.flat_w.data_ptr()
    assert torch.equal(ts.ema_w, ts.flat_w) and torch.equal(ts.ema_b, ts.flat_b) and ts.ema_updates == 0
    w0 = ts.flat_w.clone()
    refs = [R.Recurrence(ts.ema_w, 0.9, every), R.Recurrence(ts.ema_b, 0.9, every)]
    worst = 0.0
    for step in range(1, 5):
        (la, _), (lb, _) = ts.step(x, t), twin.step(x, t)
        assert float(la) == float(lb) and np.isfinite(float(la))
        assert same_bits(buffers(ts), buffers(twin)), step                   # weights, biases, moments, the 16-bit image
        applied = ts.applied_steps == step                                   # (fp16: the default scale does not overflow here)
        assert applied
        for ref, avg, p in zip(refs, (ts.ema_w, ts.ema_b), (ts.flat_w, ts.flat_b)):
            want, bound, D, updates = ref.step(p, applied)
            err = (avg.double() - want).abs()
            assert bool((err <= bound).all()), (step, float((err / bound.clamp_min(1e-300)).max()))
            worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
            assert (D is None) == bool(step % every) and ts.ema_updates == updates == step // every
    assert not torch.equal(ts.flat_w, w0) and not torch.equal(ts.ema_w, ts.flat_w) and not torch.equal(ts.ema_w, w0)
    print("%s: largest error %.3f of the accumulated bound" % ((arch, precision, optimizer, every), worst))


def test_launches_sit_between_the_last_optimizer_launch_and_the_scale_update(monkeypatch):
    x, t = batch()
    names = []
    real = L.call

    def call(name, *a):
        names.append(name)
        return real(name, *a)
    for kw, opt_entry in ((dict(precision=torch.float16), "szn_adam_step_scaled"), (dict(precision=torch.float32), "szn_adam_step")):
        ts, plain = fresh(ema=dict(decay=0.9, every=2, warmup=False), **kw), fresh(**kw)
        seqs = []
        for s in (ts, ts, plain, plain):
            del names[:]
            with monkeypatch.context() as mp:
                mp.setattr(L, "call", call)
                s.step(x, t)
            seqs.append(list(names))
        odd, even, base1, base2 = seqs
        assert odd == base1 and "szn_ema_step" not in odd                    # step 1 of every = 2: the plain step, launch for launch
        assert [n for n in even if n != "szn_ema_step"] == base2 and even.count("szn_ema_step") == 2
        i = even.index("szn_ema_step")
        assert even[i - 1] == opt_entry and even[i + 1] == "szn_ema_step"    # right behind the bias update
        if ts.dynamic:
            assert even[i + 2] == "szn_loss_scale_update"
        assert ts.ema_updates == 1


def test_overflowed_steps_skip_the_average():
    """the far-too-large loss scale of test_dynamic_loss_scale_skips_overflowed_steps_and_recovers: a numeric overflow the optimizer
    kernels skip on the device -- so does the average, and it moves on the first applied step"""
    x, t = batch()
    ts = fresh(precision=torch.float16, loss_scale=2.0 ** 40, ema=dict(decay=0.9))
    assert ts.dynamic
    aw, ab = ts.ema_w.clone(), ts.ema_b.clone()
    skipped = 0
    for _ in range(60):
        ts.step(x, t)
        if ts.applied_steps:
            break
        skipped += 1
        assert torch.equal(ts.ema_w, aw) and torch.equal(ts.ema_b, ab) and torch.equal(ts.flat_w, aw)
    assert skipped >= 1 and ts.applied_steps == 1 and ts.ema_updates == skipped + 1      # every step launched, one applied
    assert not torch.equal(ts.flat_w, aw) and not torch.equal(ts.ema_w, aw)
    # the first applied step: s = 0 on the device whatever the host's step count says -> D = 0.1
    want = R.ema_update(aw, ts.flat_w, R.ema_factor(0.9, 1, 0))
    assert bool(((ts.ema_w.double() - want).abs() <= R.ema_step_bound(aw, ts.flat_w)).all())


@pytest.mark.parametrize("arch,precision", [("fcn32s", torch.float32), ("fcn32s", torch.bfloat16), ("fcn32s", torch.float16),
                                            ("fcn8s", torch.bfloat16)], ids=["fcn32s-fp32", "fcn32s-bf16", "fcn32s-fp16", "fcn8s-bf16"])
def test_averaged_weights_is_an_exact_exchange(arch, precision):
    x, t = batch()
    ts, twin = fresh(arch, precision, ema=dict(decay=0.5)), fresh(arch, precision, ema=dict(decay=0.5))
    for _ in range(2):
        ts.step(x, t)
        twin.step(x, t)
    five = lambda s: [s.flat_w, s.flat_b, s.ema_w, s.ema_b] + ([s.flat_w_lp] if s.flat_w_lp is not None else [])
    before = [b.clone() for b in five(ts)]
    tail = None if ts.flat_w_lp is None else ts._flat_w_lp_store[ts.flat_w.numel():].clone()
    sd = ts.ema_state_dict()
    assert list(sd) == list(ts.model.state_dict()) and all(sd[k].shape == v.shape for k, v in ts.model.state_dict().items())
    assert torch.equal(sd["upscore.weight" if arch == "fcn32s" else "upscore8.weight"],                # a frozen entry: the model's
                       ts.model.state_dict()["upscore.weight" if arch == "fcn32s" else "upscore8.weight"])
    assert not torch.equal(sd["fc6.weight"], ts.model.fc6.weight)
    ref = ARCH[arch](E).load_synthetic(7, device=torch.device("cuda")).eval()
    ref.load_state_dict(sd)
    ref.set_precision(precision)
    with torch.no_grad():
        want_loss, want_pred = ref.embed_predict(x, EMB, t)
        raw_loss, _ = ts.model.embed_predict(x, EMB, t)
        with ts.averaged_weights():
            assert torch.equal(ts.flat_w, before[2]) and torch.equal(ts.ema_w, before[0])
            got_loss, got_pred = ts.model.embed_predict(x, EMB, t)
            with ts.averaged_weights():                                      # nested entry: a no-op
                assert torch.equal(ts.flat_w, before[2])
                again, _ = ts.model.embed_predict(x, EMB, t)
            assert torch.equal(ts.flat_w, before[2])                         # ... that does not end the outer block
            assert all(torch.equal(a, b) for a, b in zip(ts.ema_state_dict().values(), sd.values()))
            with pytest.raises(L.SznError):
                ts.step(x, t)
    assert float(got_loss) == float(want_loss) == float(again) and torch.equal(got_pred, want_pred)
    assert float(raw_loss) != float(got_loss)                                # the average is not the iterate here
    assert same_bits(five(ts), before)
    if tail is not None:
        assert torch.equal(ts._flat_w_lp_store[ts.flat_w.numel():], tail)
    # an exception inside the block still restores everything
    with pytest.raises(ZeroDivisionError):
        with ts.averaged_weights():
            1 / 0
    assert same_bits(five(ts), before) and not ts._ema_in
    with torch.no_grad():
        assert float(ts.model.embed_predict(x, EMB, t)[0]) == float(raw_loss)
    # training continues bit for bit
    for _ in range(2):
        (la, pa), (lb, pb) = ts.step(x, t), twin.step(x, t)
        assert float(la) == float(lb) and torch.equal(pa, pb)
    assert same_bits(five(ts) + list(ts.state["w"]), five(twin) + list(twin.state["w"]))


@pytest.mark.parametrize("fail_at", [1, 2, 3])
def test_an_entry_that_fails_half_way_is_undone(monkeypatch, fail_at):
    """the entry's first exchange, second exchange or cast of the 16-bit image raises: nothing stays exchanged"""
    x, t = batch()
    ts = fresh(precision=torch.bfloat16, ema=dict(decay=0.5))
    ts.step(x, t)
    five = lambda: [ts.flat_w, ts.flat_b, ts.ema_w, ts.ema_b, ts.flat_w_lp]
    before = [b.clone() for b in five()]
    real, seen = L.call, []

    def call(name, *a):
        seen.append(name)
        if len(seen) == fail_at:
            raise L.SznError("injected")
        return real(name, *a)
    with monkeypatch.context() as mp:
        mp.setattr(L, "call", call)
        with pytest.raises(L.SznError, match="injected"):
            with ts.averaged_weights():
                raise AssertionError("the block must not run")
    assert seen[:fail_at] == ["szn_swap_f32", "szn_swap_f32", "szn_cast"][:fail_at]
    assert same_bits(five(), before) and not ts._ema_in
    with ts.averaged_weights():                                              # and the next visit works
        assert torch.equal(ts.flat_w, before[2])
    assert same_bits(five(), before)


def test_state_dict_round_trip_and_reset():
    x, t = batch()
    ts = fresh(ema=dict(decay=0.5))
    ts.step(x, t)
    sd = ts.ema_state_dict()
    aw, ab = ts.ema_w.clone(), ts.ema_b.clone()
    ts.reset_ema()
    assert torch.equal(ts.ema_w, ts.flat_w) and ts.ema_updates == 0 and not torch.equal(ts.ema_w, aw)
    ts.load_ema_state_dict({k: v.cpu() for k, v in sd.items()})
    assert torch.equal(ts.ema_w, aw) and torch.equal(ts.ema_b, ab)
    with pytest.raises(L.SznError):
        ts.load_ema_state_dict({k: v for k, v in sd.items() if k != "fc7.bias"})
    plain = fresh()
    for call in (plain.ema_state_dict, plain.reset_ema, lambda: plain.averaged_weights().__enter__()):
        with pytest.raises(L.SznError):
            call()


def test_refusals(monkeypatch, tmp_path):
    m = models.FCN32s(E).load_synthetic(1337, device=torch.device("cuda")).eval()
    for bad in (dict(decay=1.0), dict(decay=-0.5), dict(decay=0.9, every=0), dict(decay=0.9, every=-2)):
        with pytest.raises(ValueError):
            engine.TrainStep(m, EMB, precision=torch.float32, ema=bad)
    # the sharded optimizer, on a forced one-rank exchange
    import torch.distributed as dist
    monkeypatch.setenv("SZN_SHARDED_OPT", "1")
    dist.init_process_group("gloo", store=dist.FileStore(str(tmp_path / "store"), 1), rank=0, world_size=1)
    try:
        ok = engine.TrainStep(m, EMB, precision=torch.float32, force_comm=True)
        assert ok.buckets.sharded
        m2 = models.FCN32s(E).load_synthetic(1337, device=torch.device("cuda")).eval()
        with pytest.raises(ValueError) as e:
            engine.TrainStep(m2, EMB, precision=torch.float32, force_comm=True, ema=dict(decay=0.9))
        assert "sharded" in str(e.value)
    finally:
        dist.destroy_process_group()
