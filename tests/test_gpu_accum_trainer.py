"""GPU: gradient accumulation through train.py --accum-steps and Trainer(accum_steps=), on the synthetic dataset (configuration 4:
pascal, 20-d embeddings, cosine loss, Adam; 64 x 64 images, one per iteration): an iteration stays one loader batch, the optimizer runs
on every A-th one, grad_log.csv has one row per optimizer step, a window is carried across the end of an epoch, and a run without the
flag is the run it was."""
import glob
import os
import shutil
import sys
import tempfile

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zeroshotsemanticsegmentation_amd import _lib as L  # noqa: E402
from zeroshotsemanticsegmentation_amd import engine, models, train, trainer_fcn  # noqa: E402
from zeroshotsemanticsegmentation_amd.configs import configurations  # noqa: E402
from zeroshotsemanticsegmentation_amd.synthetic_dataset import SyntheticSegmentation  # noqa: E402

COMMON = ['-c', '4', '--workers', '0']


def run_dir(d, name):
    logs = glob.glob(os.path.join(d, 'logs', name + '_CFG_*'))
    assert len(logs) == 1, logs
    return logs[0]


def rows(log, fname):
    return [r.split(',') for r in open(os.path.join(log, fname)).read().strip().split('\n')]


def run(d, name, argv):
    """train.main with the flags `argv` -> (the run's log directory, the fused steps it built, the entry points it launched)"""
    steps, names = [], []
    real_call = L.call

    class Recorded(engine.TrainStep):
        def __init__(self, *a, **kw):
            steps.append(self)
            super().__init__(*a, **kw)

    def call(name, *a):
        names.append(name)
        return real_call(name, *a)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(engine, "TrainStep", Recorded)
        mp.setattr(L, "call", call)
        train.main(COMMON + ['-dir', d, '-n', name] + argv)
    return run_dir(d, name), steps, names


@pytest.fixture(scope="module")
def runs():
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    d = tempfile.mkdtemp(prefix="szn_accum_", dir=base)
    try:
        four = ['--synthetic', '4', '64', '64', '-ve', '1']
        yield dict(d=d,
                   two=run(d, 'two', four + ['--accum-steps', '2', '--grad-stats']),
                   plain=run(d, 'plain', four),
                   one=run(d, 'one', four + ['--accum-steps', '1']),
                   span=run(d, 'span', ['--synthetic', '3', '64', '64', '-ve', '2', '--accum-steps', '2']))
    finally:
        shutil.rmtree(d, ignore_errors=True)


def test_two_iterations_per_optimizer_step(runs):
    log, steps, names = runs["two"]
    assert len(steps) == 1
    step = steps[0]
    assert step.accum_steps == 2 and step._accum == (2, True) and step.applied_steps == 2 == step.nstep and step.accum_pending == 0
    r = rows(log, 'train_log.csv')
    assert [int(x[1]) for x in r[-4:]] == [0, 1, 2, 3]                       # an iteration stays one loader batch
    assert names.count("szn_grad_accum") == 2 * 4 and names.count("szn_clip_coef") == 2
    assert names.count("szn_adam_step_clipped") == 2 * 2
    g = rows(log, 'grad_log.csv')
    assert g[0][:5] == ['epoch', 'iteration', 'grad_norm', 'clip_coef', 'clipped_steps']
    assert [(int(x[0]), int(x[1])) for x in g[1:]] == [(0, 1), (0, 3)]       # one row per boundary
    assert all(0 < float(x[2]) < float("inf") and float(x[3]) == 1.0 for x in g[1:])


def test_run_without_the_flag_is_the_run_it_was(runs):
    (plog, psteps, pnames), (olog, osteps, onames) = runs["plain"], runs["one"]
    assert pnames == onames and "szn_grad_accum" not in pnames
    assert psteps[0].acc_w is None and osteps[0].acc_w is None and osteps[0].accum_steps == 1 and psteps[0].applied_steps == 4
    assert psteps[0].fused_adam == osteps[0].fused_adam
    p, o = rows(plog, 'train_log.csv'), rows(olog, 'train_log.csv')
    assert len(p) == len(o) and [x[:-1] for x in p] == [x[:-1] for x in o]   # every column but the elapsed time
    assert sorted(os.listdir(plog)) == sorted(os.listdir(olog))
    cp = torch.load(os.path.join(plog, 'checkpoint'), map_location='cpu', weights_only=False)
    co = torch.load(os.path.join(olog, 'checkpoint'), map_location='cpu', weights_only=False)
    assert all(torch.equal(cp['model_state_dict'][k], v) for k, v in co['model_state_dict'].items())
    # the accumulated run starts from the same weights: the losses of its first window are the plain run's first loss and its own
    t = rows(runs["two"][0], 'train_log.csv')
    assert t[-4][2] == p[-4][2] and t[-3][2] != p[-3][2]


def test_a_window_spans_the_end_of_an_epoch(runs):
    log, steps, names = runs["span"]
    step = steps[0]
    r = rows(log, 'train_log.csv')
    assert [(int(x[0]), int(x[1])) for x in r[-6:]] == [(0, 0), (0, 1), (0, 2), (1, 3), (1, 4), (1, 5)]
    assert step.applied_steps == 3 and step.accum_pending == 0 and names.count("szn_grad_accum") == 2 * 6
    # SET, FINAL, SET | FINAL, SET, FINAL: the third iteration's gradient waits for the next epoch's first
    assert names.count("szn_adam_step") == 2 * 3
    assert not os.path.exists(os.path.join(log, 'grad_log.csv'))


def _trainer(tmp, config=4, loss="cos", embed=20, model=None, **kw):
    cfg = configurations[config]
    m = model if model is not None else models.FCN32s(embed if embed else 21).load_synthetic(1337, device=torch.device("cuda"))
    ds = SyntheticSegmentation(split="val", n_images=1, size=(64, 64), n_class=21, embed_dim=20, seed=1337)
    loader = torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False)
    return trainer_fcn.Trainer(cuda=True, model=m, optimizer=train.make_fcn_optimizer(m, cfg), train_loader=loader, val_loader=loader,
                               log_dir=str(tmp), dataset="pascal", max_epoch=1, tb_writer=None, pixel_embeddings=embed, loss_func=loss, **kw)


def test_trainer_keyword_and_refusals(tmp_path):
    m = models.FCN32s(20).load_synthetic(1337, device=torch.device("cuda"))
    with pytest.raises(L.SznError) as e:
        _trainer(tmp_path, model=m, fused_step=False, accum_steps=2)
    assert str(e.value) == trainer_fcn.accum_refused(True, False)
    with pytest.raises(L.SznError) as e:
        _trainer(tmp_path, model=m, loss="cross_entropy", accum_steps=2)     # cross entropy on an embedding network: autograd route
    assert str(e.value) == trainer_fcn.accum_refused(False)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError):
            _trainer(tmp_path, model=m, accum_steps=bad)
    assert _trainer(tmp_path, model=m).accum is None
    t = _trainer(tmp_path, model=m, accum_steps=4)
    assert t.accum == dict(steps=4, average=True) and t._fast_step().accum_steps == 4 and t._fast_step().grad_factor() == 0.25
    # the reference's pixel-sum cross entropy: a larger batch grows the gradient the same way, so the window's sum is used
    t = _trainer(tmp_path, config=1, loss="cross_entropy", embed=0, accum_steps=4)
    assert t.accum == dict(steps=4, average=False) and t._fast_step().grad_factor() == 1.0


def test_flag_on_another_route_raises(runs):
    with pytest.raises(L.SznError) as e:
        train.main(COMMON + ['--synthetic', '2', '64', '64', '-ve', '1', '-dir', runs["d"], '-n', 'bad', '-loss', 'cross_entropy',
                             '--accum-steps', '2'])
    assert str(e.value) == "--accum-steps: " + trainer_fcn.accum_refused(False)
