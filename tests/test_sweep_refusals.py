"""CPU: the five refusal functions of the sweeping inference rules (calibration_refused, seen_threshold_refused, seen_gate_refused,
hub_refused, conse_refused) return, for every combination of their arguments, the sentences recorded in
tests/golden/sweep_refusals.json before they were moved onto one table -- byte for byte -- and none of them builds its sentence by
editing another rule's."""
import inspect
import itertools
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEVEN = ("calibration_refused", "seen_threshold_refused", "seen_gate_refused", "hub_refused")     # the seven-argument functions


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "sweep_refusals.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", SEVEN)
def test_seven_argument_rules_reproduce_the_recorded_sentences(name):
    from zeroshotsemanticsegmentation_amd import trainer_fcn
    gold = _golden()
    fn, seen = getattr(trainer_fcn, name), set()
    assert len(gold[name]) == 2 ** 5 * 2 * 2
    for bools in itertools.product((False, True), repeat=5):
        for n_class in (21, 257):
            for verbose in (False, True):
                key = "%s:%d:%d" % ("".join(str(int(b)) for b in bools), n_class, verbose)
                want = gold["messages"][gold[name][key]]
                assert fn(*bools, n_class, verbose) == want, key
                if not verbose:
                    assert fn(*bools, n_class) == want, key                  # verbose_val defaults to False
                seen.add(want)
    assert None in seen and len(seen) == 8                                       # seven reasons and "nothing refused"


def test_conse_reproduces_the_recorded_sentences():
    from zeroshotsemanticsegmentation_amd import trainer_fcn
    gold = _golden()
    assert len(gold["conse_refused"]) == 2 ** 6
    seen = set()
    for bools in itertools.product((False, True), repeat=6):
        want = gold["messages"][gold["conse_refused"]["".join(str(int(b)) for b in bools)]]
        assert trainer_fcn.conse_refused(*bools) == want, bools
        seen.add(want)
    assert None in seen and len(seen) == 6


def test_parameter_lists_are_unchanged():
    from zeroshotsemanticsegmentation_amd import trainer_fcn
    for name in SEVEN:
        sig = inspect.signature(getattr(trainer_fcn, name))
        assert list(sig.parameters) == ["has_unseen", "embed_cfg", "forced_unseen", "test_all", "eval_views", "n_class", "verbose_val"]
        assert sig.parameters["verbose_val"].default is False
    assert list(inspect.signature(trainer_fcn.conse_refused).parameters) == ["has_unseen", "softmax_cfg", "forced_unseen", "test_all",
                                                                             "eval_views", "tuned"]


def test_no_sentence_is_built_from_another_rules_sentence():
    from zeroshotsemanticsegmentation_amd import trainer_fcn
    shared = set()
    for name in SEVEN + ("conse_refused",):
        fn = getattr(trainer_fcn, name)
        assert ".replace(" not in inspect.getsource(fn), name
        # the module-level functions the body calls: the one they share
        shared |= {n for n in fn.__code__.co_names if inspect.isfunction(getattr(trainer_fcn, n, None))}
    assert len(shared) == 1, shared
    assert ".replace(" not in inspect.getsource(getattr(trainer_fcn, shared.pop()))
