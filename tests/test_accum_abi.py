"""CPU: the gradient-accumulation surface that needs no GPU -- the prototype of include/szn.h against the ctypes binding and the three mode
constants, the host-side argument check of engine.TrainStep(accum=), the Trainer's refusal through the table, train.py's flag and the
new keywords' defaults."""
import ctypes as C
import inspect
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_ema_abi import prototype  # noqa: E402
from zeroshotsemanticsegmentation_amd import _lib, engine, train, trainer_fcn  # noqa: E402
from zeroshotsemanticsegmentation_amd.configs import configurations  # noqa: E402

CTYPE = {"long": C.c_long, "int": C.c_int, "float*": C.c_void_p, "szn_stream_t": C.c_void_p}


def test_header_prototype_matches_the_binding():
    res, args = prototype("szn_grad_accum")
    assert res == "int" and args == ["long", "float*", "float*", "int", "szn_stream_t"]
    rtype, atypes = _lib.SIGNATURES["szn_grad_accum"]
    assert rtype is C.c_int and atypes == [CTYPE[a] for a in args]


def test_mode_constants_match_the_header():
    txt = open(os.path.join(ROOT, "include", "szn.h")).read()
    for name, value in (("SET", _lib.ACCUM_SET), ("ADD", _lib.ACCUM_ADD), ("FINAL", _lib.ACCUM_FINAL)):
        assert ("#define SZN_ACCUM_%-5s %d\n" % (name, value)) in txt, name
    assert (_lib.ACCUM_SET, _lib.ACCUM_ADD, _lib.ACCUM_FINAL) == (0, 1, 2)


def test_trainstep_checks_accum_on_the_host():
    chk = engine.TrainStep._check_accum
    assert chk(dict(steps=4)) == (4, True)
    assert chk(dict(steps=1)) == (1, True)
    assert chk(dict(steps=2, average=False)) == (2, False)
    for bad in (4, None, [4], dict(), dict(average=True), dict(steps=2, mean=True), dict(steps=True), dict(steps=2.0), dict(steps="2"),
                dict(steps=None), dict(steps=0), dict(steps=-3), dict(steps=2, average=1), dict(steps=2, average=None)):
        with pytest.raises(ValueError):
            chk(bad)


def test_trainer_refusal_goes_through_the_table():
    assert trainer_fcn.accum_refused(True) is None
    for kw, key in ((dict(step_cfg=False), "config"), (dict(step_cfg=True, fused_step=False), "fused"),
                    (dict(step_cfg=True, wired=False), "wiring")):
        assert trainer_fcn.accum_refused(**kw) == dict(trainer_fcn._REFUSALS["accum"])[key]
    assert [k for k, _ in trainer_fcn._REFUSALS["accum"]] == [k for k, _ in trainer_fcn._REFUSALS["ema"]]
    for other in ("ema", "clip"):
        assert not set(dict(trainer_fcn._REFUSALS["accum"]).values()) & set(dict(trainer_fcn._REFUSALS[other]).values())


def _check(argv):
    args = train.build_parser().parse_args(argv)
    cfg = train.update_cfg_with_args(configurations[args.config], args)
    return train.check_accum(args.accum_steps, cfg)


def test_flag_accepted():
    assert _check(["-c", "18"]) is None
    assert _check(["-c", "18", "--accum-steps", "1"]) == 1
    assert _check(["-c", "18", "--accum-steps", "8"]) == 8
    for loss in ("mse", "sim_ce", "rank"):
        assert _check(["-c", "18", "-loss", loss, "--accum-steps", "2"]) == 2
    assert _check(["-c", "1", "--accum-steps", "4"]) == 4                       # the softmax configuration trains on TrainStep too
    assert train.build_parser().parse_args(["-c", "18"]).accum_steps is None


def test_flag_refused():
    with pytest.raises(_lib.SznError) as e:                                    # cross entropy on an embedding network: autograd route
        _check(["-c", "18", "-loss", "cross_entropy", "--accum-steps", "2"])
    assert str(e.value) == "--accum-steps: " + dict(trainer_fcn._REFUSALS["accum"])["config"]
    for argv, word in ((["-c", "18", "--accum-steps", "0"], "at least 1"), (["-c", "18", "--accum-steps", "-2"], "at least 1"),
                       (["-c", "19", "-r", "run", "--accum-steps", "2"], "-m train"),
                       (["-c", "18", "-m", "test_fcn", "-r", "run", "--accum-steps", "2"], "-m train")):
        with pytest.raises(Exception) as e:
            _check(argv)
        assert word in str(e.value), (argv, str(e.value))
    with pytest.raises(SystemExit):                                            # argparse: A is an integer
        train.build_parser().parse_args(["-c", "18", "--accum-steps", "2.5"])


def test_new_keywords_default_to_none():
    assert inspect.signature(engine.TrainStep.__init__).parameters["accum"].default is None
    p = inspect.signature(trainer_fcn.Trainer.__init__).parameters
    assert p["accum_steps"].default is None
    assert list(p)[-4:] == ["calibration", "calib_sweep", "eval_scales", "eval_flip"]                # the pinned tail stays
