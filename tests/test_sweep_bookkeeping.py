"""CPU: the validation sweeps' host bookkeeping (trainer_fcn._Sweep: calibration / hubness correction, ConSE, seen-mask threshold / soft
gate) reproduces tests/golden/sweep_bookkeeping.json, recorded from the three hand-written state machines it replaced: the merged
values, the index of the value in use, the 64-cap, the best pick, and the CSV text, prints and tensorboard scalars of the reports.
Driven on a bare Trainer (object.__new__) with CPU tensors: no GPU, no model forward."""
import json
import os
import sys
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

with open(os.path.join(ROOT, "tests", "golden", "sweep_bookkeeping.json")) as _f:
    GOLD = json.load(_f)
K, VAL_UNSEEN = GOLD["n_class"], GOLD["val_unseen"]
RULES = ("calib", "hub", "conse", "seen", "gate")
CASES = {c["name"]: c for c in GOLD["cases"]}


class _Scalars(object):
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, value, step):
        self.rows.append([tag, float(value), int(step)])


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(1, 1)


def _trainer(rule, sweep, used, log_dir, rank=0):
    """a Trainer with the attributes the sweeps read, configured for `rule` with the candidates `sweep` and the value in use `used`"""
    from zeroshotsemanticsegmentation_amd import trainer_fcn
    t = object.__new__(trainer_fcn.Trainer)
    t.log_dir, t.n_class, t.val_unseen, t.unseen = str(log_dir), K, VAL_UNSEEN, VAL_UNSEEN
    t.epoch, t.iteration, t.tb_writer, t.rank, t.device = GOLD["epoch"], GOLD["iteration"], _Scalars(), rank, torch.device("cpu")
    t.calibration = t.calib_sweep = t.hub = t.conse = t.conse_sweep = t.seen_threshold = t.seen_sweep = t.seen_gate = None
    t.best_gamma = t.best_harmonic_mean_iu = t.best_seen_tau = t.best_seen_harmonic_mean_iu = None
    t.best_conse_gamma = t.best_conse_harmonic_mean_iu = t.last_hub_skew = None
    sw = None if sweep is None else np.asarray(sweep, dtype=np.float32)
    u = None if used is None else float(np.float32(used))
    if rule in ("calib", "hub"):
        t.calibration, t.calib_sweep, t.hub = u, sw, dict(GOLD["hub"]) if rule == "hub" else None
    elif rule == "conse":
        t.conse, t.conse_sweep = dict(top=3, dim=20, gamma=0.0 if u is None else u), sw
    else:
        t.seen_threshold, t.seen_sweep, t.seen_gate = u, sw, dict(GOLD["gate"]) if rule == "gate" else None
    t.model, t.val_loader, t.visualize, t.verbose_val, t.best_mean_iu, t._step = _Net(), [], 0, False, 0, None     # what _validate reads
    t._init_sweeps()
    return t


def _record(t, rule):
    return {"calib": t._calib, "hub": t._calib, "conse": t._conse, "seen": t._seen, "gate": t._seen}[rule]


def _best(t, rule):
    return {"calib": (t.best_gamma, t.best_harmonic_mean_iu), "hub": (t.best_gamma, t.best_harmonic_mean_iu),
            "conse": (t.best_conse_gamma, t.best_conse_harmonic_mean_iu), "seen": (t.best_seen_tau, t.best_seen_harmonic_mean_iu),
            "gate": (t.best_seen_tau, t.best_seen_harmonic_mean_iu)}[rule]


def _split(h):
    """the {all, seen, unseen} histograms validation keeps, from one (K,K) histogram"""
    un = np.zeros(K, dtype=bool)
    un[VAL_UNSEEN] = True
    return [h, np.where(un[:, None], 0, h), np.where(un[:, None], h, 0)]


def test_the_fixture_holds_the_cases_it_should():
    assert len(GOLD["cases"]) >= 36 and len(CASES) == len(GOLD["cases"])
    kinds = {n.split("_")[-1] for n in CASES if n.startswith("seeded")}
    assert kinds == {"inside", "outside", "none"}
    assert {c["report"]["rule"] for c in GOLD["cases"] if c["report"]} == set(RULES)
    nan = [c for n, c in CASES.items() if n.startswith("all_nan")]
    assert len(nan) == 5 and all(c["report"]["best"] is None and "nan" in c["report"]["csv"] for c in nan)
    tie = [c for n, c in CASES.items() if n.startswith("tie_")]
    assert tie and all(c["report"]["best"][0] == -0.5 for c in tie)           # |-0.5| == |0.5|: the first of the two stays
    assert all("error" in r for r in CASES["cap64_outside"]["rules"].values())
    assert all(len(r["all"]) == 64 for r in CASES["cap64_inside"]["rules"].values())


@pytest.mark.parametrize("name", sorted(CASES))
def test_values_index_and_cap(name, tmp_path):
    from zeroshotsemanticsegmentation_amd._lib import SznError
    case = CASES[name]
    for rule in RULES:
        want = case["rules"][rule]
        t = _trainer(rule, case["sweep"], case["used"], tmp_path)
        rec = _record(t, rule)
        if "error" in want:
            with pytest.raises(SznError) as e:
                rec.begin()
            assert [type(e.value).__name__, str(e.value)] == want["error"], rule
            continue
        # outside a sweep: the value in use alone, at index 0 (no calibration: no index)
        assert rec.hist is None and rec.values() == want["outside"] and rec.index() == want["outside_index"], rule
        rec.begin()
        assert rec.values() is rec.all and rec.all.dtype == np.float32 and rec.all.tolist() == want["all"], rule
        assert rec.index() == want["index"], rule
        G = len(want["all"])
        assert rec.hist.dtype == torch.int64 and tuple(rec.hist.shape) == (G, K, K) and not rec.hist.any(), rule
        rec.hist[G - 1, 1, 2] = 7
        out = rec.finish(1)
        assert isinstance(out, np.ndarray) and out.shape == (G, K, K) and out.sum() == 7 and out[G - 1, 1, 2] == 7, rule
        assert rec.hist is None and rec.finish(1) is None and rec.values() == want["outside"], rule


def test_without_a_calibration_there_is_no_index():
    t = _trainer("calib", [-0.5, 0.5], None, ".")
    assert t._calib.index() is None and t._calib.values() == [None]
    t._calib.begin()
    assert t._calib.index() is None and t._calib.all.tolist() == [-0.5, 0.5]      # nothing joins the sweep
    t = _trainer("hub", [-0.5, 0.5], None, ".")                                    # the hubness correction reports gamma = 0
    assert t._calib.index() == 0 and t._calib.values() == [0.0]
    t._calib.begin()
    assert t._calib.index() == 1 and t._calib.all.tolist() == [-0.5, 0.0, 0.5]
    for rule in ("seen", "gate", "conse"):
        t = _trainer(rule, None, None, ".")
        assert _record(t, rule).values() == [0.0] and _record(t, rule).index() == 0
    t = _trainer("seen", None, 0.75, ".")
    assert t._seen.values() == [0.75] and t._seen.index() == 0
    # the public attributes are read when asked, not copied at construction
    t.seen_threshold = -0.25
    assert t._seen.values() == [-0.25]


@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if c["report"]))
def test_reports(name, tmp_path, capsys):
    case = CASES[name]
    want, rule = case["report"], case["report"]["rule"]
    t = _trainer(rule, case["sweep"], case["used"], tmp_path)
    rec = _record(t, rule)
    rec.begin()
    rec.finish(1)
    hist = np.asarray(case["hist"], dtype=np.int64)[:rec.all.size]
    capsys.readouterr()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                     # nanmean of an empty slice in the all-NaN cases
        picked = rec.scan(hist)[1]
        if rule == "hub":
            t._hub_report(_split(hist[case["rules"][rule]["index"]]), hist)
        elif rule == "gate":
            t._gate_report(hist)
        else:
            rec.report(hist)
    assert capsys.readouterr().out == want["out"]
    assert os.listdir(str(tmp_path)) == [want["file"]]
    with open(os.path.join(str(tmp_path), want["file"])) as f:
        assert f.read() == want["csv"]
    assert (None if picked is None else list(picked)) == want["best"]
    assert _best(t, rule) == (tuple(want["best"]) if want["best"] else (None, None))
    assert t.tb_writer.rows == want["scalars"] and t.last_hub_skew == want["hub_skew"]


def test_the_hubness_report_without_a_sweep_writes_the_used_row_alone(tmp_path, capsys):
    t = _trainer("hub", None, 0.25, tmp_path)
    h = np.arange(K * K, dtype=np.int64).reshape(K, K)
    t._hub_report(_split(h), None)
    rows = open(os.path.join(str(tmp_path), "hub_log.csv")).read().splitlines()
    assert len(rows) == 2 and rows[1].startswith("3,17,used,zscore,0.5,0.05,0.25,")
    assert t.best_gamma is None and capsys.readouterr().out == ""


@pytest.mark.parametrize("name", ["seeded01_outside", "seeded05_none", "tie_hub", "cap64_outside", "cap64_inside"])
def test_validate_begins_and_finishes_every_sweep(name, tmp_path):
    """_validate on an empty loader (a rank that writes nothing): the sweeps begin with the recorded values and are over afterwards"""
    from zeroshotsemanticsegmentation_amd._lib import SznError
    case = CASES[name]
    for rule in RULES:
        want = case["rules"][rule]
        t = _trainer(rule, case["sweep"], case["used"], tmp_path, rank=1)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            if "error" in want:
                with pytest.raises(SznError) as e:
                    t._validate(rule in ("seen", "gate"))
                assert str(e.value) == want["error"][1], rule
                continue
            t._validate(rule in ("seen", "gate"))
        for rec in t._sweeps:
            assert rec.hist is None
            assert (rec.all.tolist() == want["all"]) if rec is _record(t, rule) else (rec.all is None), rule
    assert os.listdir(str(tmp_path)) == []
