"""CPU: the host checks the five sweep heads share (heads.calib, hub, conse, seen_sweep, soft_gate) raise SznError with each head's own
sentence before anything is launched -- CPU tensors at the geometry the *_abi tests use (B 1, map 2 x 2 x 24, E 20, K 21, image 33 x 47,
stride 32).  Where a call passes every check it reaches exactly one L.call, which is recorded instead of run."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, h, w, LD, E, K, H, W = 1, 2, 2, 24, 20, 21, 33, 47
UNSEEN = (2, 5)
HEADS = ("calib", "hub", "conse", "seen_sweep", "soft_gate")
NOUN = {"calib": "gammas", "hub": "gammas", "conse": "gammas", "seen_sweep": "taus", "soft_gate": "taus"}
VALUES_WHO = {"gammas": "calibration", "taus": "seen sweep"}
ENTRY = {"calib": "szn_calib_head", "hub": "szn_hub_head", "conse": "szn_conse_head", "seen_sweep": "szn_seen_sweep_head",
         "soft_gate": "szn_soft_gate_head"}
MARGIN_HEADS = ("seen_sweep", "soft_gate")


@pytest.fixture(scope="module")
def lib():
    """the workspace-size queries run in the library (host code only)"""
    import __graft_entry__ as g
    from zeroshotsemanticsegmentation_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        g.build()
    return L.load()


@pytest.fixture
def calls(monkeypatch):
    """L.call recorded, not run: a call that passes the host checks ends here"""
    from zeroshotsemanticsegmentation_amd import _lib as L
    seen = []
    monkeypatch.setattr(L, "call", lambda name, *args: seen.append((name, args)))
    monkeypatch.setattr(L, "stream_ptr", lambda: None)
    return seen


def _fmap():
    return torch.zeros(B, h, w, LD)


def _emb():
    return torch.ones(K, E)


def _target():
    return torch.zeros(B, H, W, dtype=torch.int64)


def _run(head, fmap=None, emb=None, values=(-0.25, 0.0, 0.25), stride=32, **kw):
    """heads.<head> with good arguments except those given"""
    from zeroshotsemanticsegmentation_amd import heads
    fmap = _fmap() if fmap is None else fmap
    emb = _emb() if emb is None else emb
    if head == "calib":
        return heads.calib(stride, fmap, emb, H, W, UNSEEN, values, **kw)
    if head == "hub":
        return heads.hub(stride, fmap, emb, H, W, UNSEEN, torch.zeros(B, K, 2), values, **kw)
    if head == "conse":
        return heads.conse(stride, fmap, emb, H, W, UNSEEN, 3, values, **kw)
    margin = torch.zeros(B, H, W)
    if head == "seen_sweep":
        return heads.seen_sweep(stride, fmap, emb, H, W, UNSEEN, margin, values, **kw)
    return heads.soft_gate(stride, fmap, emb, H, W, UNSEEN, margin, values, 0.1, 1.0, **kw)


def _refused(sentence, head, **kw):
    from zeroshotsemanticsegmentation_amd._lib import SznError
    with pytest.raises(SznError) as e:
        _run(head, **kw)
    assert str(e.value) == sentence, (head, kw.keys())


@pytest.mark.parametrize("head", HEADS)
def test_the_shared_checks_raise_each_heads_own_sentence(head, lib, calls):
    noun = NOUN[head]
    # the map: contiguous fp32
    for bad in (torch.zeros(B, h, w, 2 * LD)[..., ::2], _fmap().half(), _fmap().double()):
        assert tuple(bad.shape) == (B, h, w, LD)
        _refused("%s: the map must be a contiguous fp32 (B,h,w,C) tensor" % head, head, fmap=bad, pred_index=0)
    # what to compute
    _refused("%s: a histogram needs the target" % head, head, hist=torch.zeros(3, K, K, dtype=torch.int64), pred_index=0)
    nothing = "%s: nothing to compute (no target for a histogram, no pred_index for a prediction%s)"
    _refused(nothing % (head, ", no eff" if head == "soft_gate" else ""), head)
    for bad in (-1, 3):
        _refused("%s: pred_index %r outside [0, 3)" % (head, bad), head, pred_index=bad)
        _refused("%s: pred_index %r outside [0, 3)" % (head, bad), head, pred_index=bad, target=_target())
    _refused("%s: pred_index 1 outside [0, 1)" % head, head, values=[0.5], pred_index=1)
    # the histogram the caller brings
    for bad in (torch.zeros(3, K, K, dtype=torch.int32), torch.zeros(3, K, K), torch.zeros(2, K, K, dtype=torch.int64),
                torch.zeros(3, K, K + 1, dtype=torch.int64), torch.zeros(3 * K * K, dtype=torch.int64),
                torch.zeros(3, K, 2 * K, dtype=torch.int64)[..., ::2]):
        _refused("%s: hist must be a contiguous int64 (3,%d,%d) tensor on cpu" % (head, K, K), head, target=_target(), hist=bad)
    # a geometry the head does not take
    _refused("%s: bad geometry (stride 16, B 1, map 2 x 2, E %d, K %d, 3 %s)" % (head, E, K, noun), head, stride=16, pred_index=0)
    # the values: 1 to 64, finite, strictly ascending as float32
    who = VALUES_WHO[noun]
    _refused("%s: 0 %s, between 1 and 64 are taken" % (who, noun), head, values=[], pred_index=0)
    _refused("%s: 65 %s, between 1 and 64 are taken" % (who, noun), head, values=np.arange(65), pred_index=0)
    for bad in ([0.25, 0.0], [0.0, 0.0], [0.0, 1e-46], [0.0, float("inf")], [float("nan"), 0.0]):
        got = np.asarray(bad, dtype=np.float32).tolist()
        _refused("%s: the %s must be finite and strictly ascending as float32 (got %r)" % (who, noun, got), head, values=bad, pred_index=0)
    assert calls == []                                            # nothing was launched on the way


@pytest.mark.parametrize("head", HEADS)
def test_the_checks_come_in_the_old_order(head, lib, calls):
    """the first failing check speaks: map, values, hist without target, nothing to compute, pred_index, hist, geometry"""
    noun, who = NOUN[head], VALUES_WHO[NOUN[head]]
    bad_hist = torch.zeros(1, dtype=torch.int64)
    _refused("%s: the map must be a contiguous fp32 (B,h,w,C) tensor" % head, head, fmap=_fmap().half(), values=[], hist=bad_hist)
    _refused("%s: 0 %s, between 1 and 64 are taken" % (who, noun), head, values=[], hist=bad_hist, pred_index=9)
    _refused("%s: a histogram needs the target" % head, head, hist=bad_hist, pred_index=9)
    _refused("%s: pred_index 9 outside [0, 3)" % head, head, target=_target(), hist=bad_hist, pred_index=9, stride=16)
    _refused("%s: hist must be a contiguous int64 (3,%d,%d) tensor on cpu" % (head, K, K), head, target=_target(), hist=bad_hist, stride=16)
    assert calls == []


@pytest.mark.parametrize("head", HEADS)
def test_a_good_call_reaches_one_launch(head, lib, calls):
    hist = torch.zeros(3, K, K, dtype=torch.int64)
    out = _run(head, target=_target(), hist=hist, pred_index=2)
    assert out[0] is hist and tuple(out[1].shape) == (B, H, W) and out[1].dtype == torch.int64
    assert [c[0] for c in calls] == [ENTRY[head]]
    args = calls[0][1]
    assert args[:4] == (32, B, h, w) and 3 in args and 2 in args           # G and the pred_index, as given
    del calls[:]
    out = _run(head, pred_index=0)                                         # a prediction alone: no histogram is made up
    assert out[0] is None and out[1] is not None and -1 not in calls[0][1][-6:]
    del calls[:]
    out = _run(head, target=_target())                                     # a histogram alone: zeros, and pred_index -1 goes down
    assert out[1] is None and out[0].dtype == torch.int64 and tuple(out[0].shape) == (3, K, K) and -1 in calls[0][1]


def test_soft_gate_counts_eff_as_something_to_compute(lib, calls):
    hist, pred, eff = _run("soft_gate", want_eff=True)
    assert hist is None and pred is None and eff.dtype == torch.float32 and tuple(eff.shape) == (B, H, W)
    assert [c[0] for c in calls] == ["szn_soft_gate_head"]


def _workspace(head, fmap, emb, nbytes=None, ran_on=None, emb_of=None):
    """a Workspace as the embedding head leaves it after running on `ran_on` with `emb_of` (no device: the keys are set by hand)"""
    from zeroshotsemanticsegmentation_amd import heads
    ws = heads.Workspace(fmap.device)
    ws.get(nbytes)
    ran_on = fmap if ran_on is None else ran_on
    emb_of = emb if emb_of is None else emb_of
    ws.tables = heads.Workspace.map_key(32, ran_on)
    ws.prep = (ws.buf.data_ptr(), emb_of.data_ptr(), emb_of._version, K, E)
    return ws


@pytest.mark.parametrize("head", MARGIN_HEADS)
def test_ws_must_be_the_workspace_of_this_very_map(head, lib, calls):
    from zeroshotsemanticsegmentation_amd import heads
    fmap, emb = _fmap(), _emb()
    query = heads.seen_sweep_workspace_bytes if head == "seen_sweep" else heads.soft_gate_workspace_bytes
    nbytes = query(32, fmap, emb, 3)
    assert nbytes > 0
    sentence = ("%s: ws must be the Workspace in which the embedding head last ran on this very map and embedding matrix, %d bytes or more"
                % (head, nbytes))
    good = dict(fmap=fmap, emb=emb, target=_target(), pred_index=1)
    # the control: the workspace of this map and matrix is taken, and the tabled entry point runs in its buffer
    ws = _workspace(head, fmap, emb, nbytes)
    _run(head, ws=ws, **good)
    assert [c[0] for c in calls] == [ENTRY[head] + "_tabled"]
    del calls[:]
    _refused(sentence, head, ws=heads.Workspace(fmap.device), **good)                       # never ran: no buffer
    never = heads.Workspace(fmap.device)
    never.get(nbytes)
    _refused(sentence, head, ws=never, **good)                                               # a buffer, but no head ran in it
    _refused(sentence, head, ws=_workspace(head, fmap, emb, nbytes - 1), **good)             # too small
    _refused(sentence, head, ws=_workspace(head, fmap, emb, nbytes, ran_on=_fmap()), **good)         # another map
    _refused(sentence, head, ws=_workspace(head, fmap, emb, nbytes, emb_of=_emb()), **good)          # another embedding tensor
    stale = _workspace(head, fmap, emb, nbytes)
    fmap.add_(1.0)                                                                           # the same map, written since
    _refused(sentence, head, ws=stale, **good)
    stale = _workspace(head, fmap, emb, nbytes)
    emb.mul_(2.0)
    _refused(sentence, head, ws=stale, **good)
    stale = _workspace(head, fmap, emb, nbytes)
    stale.invalidate()
    _refused(sentence, head, ws=stale, **good)
    grown = _workspace(head, fmap, emb, nbytes)
    grown.get(nbytes + 16)                                                                   # a new buffer: the tables are gone
    _refused(sentence, head, ws=grown, **good)
    assert calls == []
    # the geometry check comes first, whatever the workspace
    _refused("%s: bad geometry (stride 16, B 1, map 2 x 2, E %d, K %d, 3 taus)" % (head, E, K), head, stride=16,
             ws=heads.Workspace(fmap.device), **good)


def test_holds_compares_the_key_prepared_writes(lib, calls):
    """Workspace.prepared and Workspace.holds build the embedding key with the same code: what one wrote the other accepts"""
    from zeroshotsemanticsegmentation_amd import heads
    fmap, emb = _fmap(), _emb()
    ws = heads.Workspace(fmap.device)
    assert not ws.holds(16, 32, fmap, emb)
    buf = ws.prepared(64, emb, K, E, None)
    assert buf is ws.buf and [c[0] for c in calls] == ["szn_fused_head_prepare"]
    ws.prepared(64, emb, K, E, None)
    assert len(calls) == 1                                       # the same key: the tables stay
    assert not ws.holds(64, 32, fmap, emb)                       # prepared, but no head has run on a map yet
    ws.tables = heads.Workspace.map_key(32, fmap)                # (what embed() records after its launch)
    assert ws.holds(64, 32, fmap, emb) and ws.holds(1, 32, fmap, emb)
    assert not ws.holds(65, 32, fmap, emb) and not ws.holds(64, 8, fmap, emb)
    assert not ws.holds(64, 32, _fmap(), emb) and not ws.holds(64, 32, fmap, _emb())
    emb.add_(1.0)
    assert not ws.holds(64, 32, fmap, emb)
    ws.prepared(64, emb, K, E, None)
    assert len(calls) == 2 and ws.holds(64, 32, fmap, emb)


def test_one_body_two_names():
    from zeroshotsemanticsegmentation_amd import heads
    from zeroshotsemanticsegmentation_amd._lib import SznError
    for fn, who, noun in ((heads.calib_gammas, "calibration", "gammas"), (heads.seen_sweep_taus, "seen sweep", "taus")):
        out = fn([0.5, 1, 2.25])
        assert out.dtype == np.float32 and out.flags["C_CONTIGUOUS"] and out.tolist() == [0.5, 1.0, 2.25]
        assert fn(np.float64(3)).tolist() == [3.0] and len(fn(np.arange(64))) == 64
        for bad, why in (([], "%s: 0 %s, between 1 and 64 are taken"), (np.arange(65), "%s: 65 %s, between 1 and 64 are taken"),
                         ([1.0, 0.5], "%s: the %s must be finite and strictly ascending as float32 (got [1.0, 0.5])"),
                         ([float("nan")], "%s: the %s must be finite and strictly ascending as float32 (got [nan])")):
            with pytest.raises(SznError) as e:
                fn(bad)
            assert str(e.value) == why % (who, noun)
    for fn, who in ((heads.pseudo_permille, "pseudo labels"), (heads.ohem_permille, "ohem")):
        assert [fn(k) for k in (1, 1.0, 0.3, 0.0004, 0.0005001, 0.9996)] == [1000, 1000, 300, 1, 1, 1000]
        for bad, why in ((0, "%s: keep must lie in (0, 1], got 0"), (1.5, "%s: keep must lie in (0, 1], got 1.5"),
                         (float("nan"), "%s: keep must lie in (0, 1], got nan"), ("x", "%s: keep must be a number in (0, 1], got 'x'"),
                         (None, "%s: keep must be a number in (0, 1], got None")):
            with pytest.raises(SznError) as e:
                fn(bad)
            assert str(e.value) == why % who
