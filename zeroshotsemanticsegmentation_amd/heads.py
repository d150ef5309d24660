"""heads.py -- the host side of the fused heads: every call into szn_fused_head_grouped[_prepared], szn_fused_mse_head[_prepared],
szn_fused_ce_head and szn_seenmask_head_k goes through here (models.FCN32s / FCN8s predict methods, engine.TrainStep, engine.SeenmaskStep).

  embed     the embedding head, kind "cos" | "mse" | "sim_ce" | "rank" (wrappers cosine / cosine_predict, mse / mse_predict,
            sim_ce / sim_ce_predict, rank / rank_predict):
  cosine    loss, stats, nearest-embedding prediction and d(map) from an NHWC map: stride 32 on the 1/32 map, stride 8 on FCN8s'
            1/8 fused map (fp32).  Group mode 0 = plain (szn_fused_head_grouped launches exactly what szn_fused_head_strided
            launches, bit for bit), 1 = seen / unseen group from the seen-mask prediction, 2 = forced unseen (group from the target).
  mse       the same head with the MSE embedding loss (szn_fused_mse_head): same arguments, same prediction bit for bit, same
            Workspace tables; loss, stats and d(map) are those of sum |s - e_label|^2 / N_b.
  sim_ce    the same head with the similarity cross-entropy loss (szn_fused_simce_head): a softmax over the cosines of the classes
            outside `exclude`, divided by `temperature`; same prediction bit for bit, same Workspace tables.
  rank      the same head with the hinge ranking loss (szn_fused_rank_head, DeViSE): the label's cosine must beat the cosine of every
            other class outside `exclude` by `margin`; `hardest` keeps the hardest negative alone.  Same prediction, same tables.
  sim_ce_bias  sim_ce with QFSL's unseen-bias term (szn_fused_simce_bias_head): embed("sim_ce", ..., bias=dict(unseen=, weight=,
            hidden=HIDDEN_LABEL)); a pixel labelled `hidden` adds weight * -log sum_{u in unseen} softmax_u over all classes.
  ce        the softmax cross-entropy head, stride 32 or 8.
  seenmask  the x32 seen-mask head on the 1/32 map: training, predict and pred-only (group map) calls.
  ms        multi-scale / mirrored inference: the views of an input (szn_resize_flip_f32) and the view-ensemble head (szn_ms_head),
            which reads the maps of all views and writes one prediction.
  calib     calibrated stacking (szn_calib_head): a penalty gamma on every seen class, swept over up to 64 values in one pass --
            per gamma a confusion histogram, for one of them the prediction.
  hub       hubness correction (szn_hub_stats, szn_hub_head): per image and class the mean (and spread) of the class's similarity over the
            image's pixels is taken off before calib's rule; same gammas, histograms and prediction.
  conse     ConSE zero-shot inference for the softmax network (szn_conse_head): the top-T seen-class softmax mixes class embeddings,
            the nearest class by cosine wins, calib's gamma between the groups, swept in one pass; or forced by the target.
  seen_sweep  full SZN inference with a threshold on the seen-mask logit margin (szn_seenmask_margin, szn_seen_sweep_head): the grouped
            head's class assignment with the group decided by margin > tau, up to 64 taus in one pass.
  soft_gate   the same route with a probabilistic gate (szn_soft_gate_head): p(seen) = sigmoid(margin - tau) times a softmax over the cosines
            inside each group, which is a per-pixel adaptive threshold on the margin; same sweep, same workspace.
  pseudo    self-training pseudo labels (szn_pseudo_head): the calibrated prediction labels the most confident share of the hidden
            pixels per unseen class; the relabelled target is what a training head then reads.
  ohem      hard-pixel mining (szn_ohem_head): per image the labelled pixels with the lowest own-class cosine keep their label, the
            others read OHEM_DROP_LABEL; the relabelled target is what a training head then reads.
  class_proto  class prototypes by masked average pooling (szn_class_proto): per class the sum of the upsampled score's unit (or raw)
            vectors over the pixels a label map gives it, and the pixel counts; utils.blend_prototypes turns them into adapted embeddings.

The crop belongs to the stride (32: CROP, reference models.py:147; 8: CROP_UP8, FCN8s' upscore8).  A call without a `Workspace`
allocates its scratch and builds the embedding tables itself (the predict methods); TrainStep keeps one `Workspace` across steps.
"""
import torch

from . import _lib as L
from .datasets import HIDDEN_LABEL

CROP = 19            # models.py:147
CROP_UP8 = 31        # FCN8s upscore8 (public pytorch-fcn definition)
_CROP = {32: CROP, 8: CROP_UP8}


class Workspace(object):
    """a head workspace kept across calls, plus the embedding tables szn_fused_head_prepare wrote to its head.  The tables are
    rebuilt for a new buffer, a new embedding tensor or an in-place torch write into it (_version), and after invalidate() (a raw
    kernel writing into the tensor does not bump _version, and a new tensor may reuse the old one's address).  `tables` names the map
    whose embedding head ran here last (embed() records it): seen_sweep(ws=) reuses that call's tables for the same map only."""

    def __init__(self, device):
        self.device, self.buf, self.prep, self.tables = device, None, None, None

    def get(self, nbytes):
        if self.buf is None or self.buf.numel() < nbytes:
            self.buf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self.tables = None
        return self.buf

    def invalidate(self):
        self.prep = self.tables = None

    @staticmethod
    def map_key(stride, fmap):
        return (stride, fmap.data_ptr(), fmap._version, tuple(fmap.shape))

    def _prep_key(self, emb):
        K, E = emb.shape
        return (self.buf.data_ptr(), emb.data_ptr(), emb._version, K, E)

    def prepared(self, nbytes, emb, K, E, stream):
        ws = self.get(nbytes)
        key = self._prep_key(emb)
        if self.prep != key:
            L.call("szn_fused_head_prepare", E, K, L.ptr(emb), L.ptr(ws), stream)
            self.prep = key
        return ws

    def holds(self, nbytes, stride, fmap, emb):
        """is this the Workspace, `nbytes` or more, in which the embedding head last ran on this very map and embedding matrix"""
        return (self.buf is not None and self.buf.numel() >= nbytes and self.tables == Workspace.map_key(stride, fmap)
                and self.prep == self._prep_key(emb))


def _scratch(nbytes, device):
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def embeddings(emb, n_class, device, fused=True):
    """the K x E class-embedding matrix as a contiguous fp32 tensor on `device`; E must be the model's n_class and, for the fused
    head (fused=True), K <= MAX_CLASSES"""
    emb = torch.as_tensor(emb).to(device, torch.float32).contiguous()
    K, E = emb.shape
    if E != n_class:
        raise L.SznError("embedding dimension %d != model n_class %d" % (E, n_class))
    if fused and K > L.MAX_CLASSES:
        raise L.SznError("the fused head holds at most %d classes, got %d: use forward() + utils" % (L.MAX_CLASSES, K))
    return emb


def seen_set(who, n_class, unseen):
    """the class set `label is one of the n_class classes and not in unseen` (trainer_seenmask.py:53-56)"""
    if n_class > L.MAX_CLASSES:
        raise L.SznError("%s: at most %d classes (szn_class_set), got %d" % (who, L.MAX_CLASSES, n_class))
    return L.class_set(k for k in range(n_class) if k not in set(unseen))


def _outputs(B, H, W, device, target):
    """(pred, target as int64, loss) of a forward-only call: target and loss are None without a target"""
    pred = torch.empty(B, H, W, dtype=torch.int64, device=device)
    if target is None:
        return pred, None, None
    return pred, target.to(device=device, dtype=torch.int64).contiguous(), torch.empty(1, device=device)


# ---- embedding heads (cosine | mse | sim_ce | rank) -------------------------------------------------------------------------
_EMBED_ENTRY = {"cos": "szn_fused_head_grouped", "mse": "szn_fused_mse_head",      # all share workspace and prepare step
                "sim_ce": "szn_fused_simce_head", "rank": "szn_fused_rank_head"}
SIM_TEMPERATURE = 0.1        # the default of train.py --sim-temperature: a hyper-parameter default, not a tuned value
RANK_MARGIN = 0.1            # the default of train.py --rank-margin: DeViSE's value, a hyper-parameter default, not a tuned value


def embed_kind(loss):
    """the embedding heads' loss argument checked: "cos" | "mse" | "sim_ce" | "rank" """
    if loss not in _EMBED_ENTRY:
        raise L.SznError("embedding head: loss must be 'cos', 'mse', 'sim_ce' or 'rank', got %r" % (loss,))
    return loss


def _sim_args(kind, exclude, temperature):
    """the two extra C arguments of kind "sim_ce" (exclude: None or an iterable of classes; temperature: None = SIM_TEMPERATURE);
    an error for the other kinds"""
    if kind != "sim_ce":
        if exclude is not None or temperature is not None:
            raise L.SznError("embedding head: exclude / temperature belong to loss 'sim_ce', not %r" % (kind,))
        return ()
    return (L.class_set(exclude), float(SIM_TEMPERATURE if temperature is None else temperature))


def _rank_args(kind, exclude, margin, hardest):
    """the three extra C arguments of kind "rank" (exclude: None or an iterable of classes; margin: None = RANK_MARGIN; hardest:
    None = False); margin / hardest are an error for the other kinds (their exclude is _sim_args' business)"""
    if kind != "rank":
        if margin is not None or hardest is not None:
            raise L.SznError("embedding head: margin / hardest belong to loss 'rank', not %r" % (kind,))
        return ()
    return (L.class_set(exclude), float(RANK_MARGIN if margin is None else margin), int(bool(hardest)))


def _loss_args(kind, exclude, temperature, margin, hardest):
    """the extra C arguments of `kind` between group_map and loss; a setting that belongs to another kind is an error"""
    if kind == "rank":
        if temperature is not None:
            raise L.SznError("embedding head: temperature belongs to loss 'sim_ce', not 'rank'")
        return _rank_args(kind, exclude, margin, hardest)
    return _sim_args(kind, exclude, temperature) + _rank_args(kind, exclude, margin, hardest)


def bias_args(kind, bias, K):
    """the three extra C arguments of the bias term after sim_ce's (bias: None | dict(unseen=classes, weight=lambda, hidden=label,
    default HIDDEN_LABEL)), checked on the host: kind "sim_ce" only, unseen some but not all of [0, K), weight finite > 0, hidden < -1"""
    import math
    if bias is None:
        return ()
    if kind != "sim_ce":
        raise L.SznError("embedding head: the bias term belongs to loss 'sim_ce', not %r" % (kind,))
    unknown = sorted(set(bias) - {"unseen", "weight", "hidden"})
    if unknown or "unseen" not in bias or "weight" not in bias:
        raise L.SznError("bias loss: bias = dict(unseen=classes, weight=lambda[, hidden=label]), got keys %r" % (sorted(bias),))
    try:
        unseen = sorted(set(int(k) for k in bias["unseen"]))
        weight = float(bias["weight"])
        hidden = int(bias.get("hidden", HIDDEN_LABEL))
    except (TypeError, ValueError):
        raise L.SznError("bias loss: unseen must be class indices, weight a number, hidden an integer (got %r)" % (bias,))
    if not unseen or unseen[0] < 0 or unseen[-1] >= K or len(unseen) >= K:
        raise L.SznError("bias loss: unseen must name some, not all, classes of [0, %d) (got %r)" % (K, unseen))
    if not (math.isfinite(weight) and weight > 0.0):
        raise L.SznError("bias loss: weight must be a finite number > 0 (got %r)" % (bias["weight"],))
    if hidden >= -1:
        raise L.SznError("bias loss: the hidden label must lie below -1 (got %r): -1 and the class labels are taken" % (hidden,))
    return (L.class_set(unseen), weight, hidden)


def embed(kind, stride, fmap, emb, H, W, pred, target=None, loss=None, stats=None, dmap=None, mode=0, classes=None, gmap=None,
          ws=None, stream=None, exclude=None, temperature=None, bias=None, margin=None, hardest=None):
    """szn_fused_head_grouped (kind "cos") / szn_fused_mse_head (kind "mse") / szn_fused_simce_head (kind "sim_ce", with exclude = the
    classes that do not compete and temperature) / szn_fused_rank_head (kind "rank", with exclude, margin and hardest) on the contiguous NHWC map `fmap` (the E embedding channels first).  target / loss / stats go together; dmap (zero-padded, [E, ld) stays untouched) receives d loss / d fmap in its
    dtype.  classes = the unseen class set (L.class_set) of modes 1 / 2, gmap the group map of mode 1.  ws: a Workspace (its
    embedding tables are reused, whichever kind wrote them) or None.  bias (kind "sim_ce" only): dict(unseen=, weight=, hidden=) routes
    to szn_fused_simce_bias_head (bias_args)."""
    B, h, w, ld = fmap.shape
    K, E = emb.shape
    st = L.stream_ptr() if stream is None else stream
    nbytes = L.load().szn_fused_head_workspace_bytes(B, h, w, E, K)
    fn = _EMBED_ENTRY[kind]
    sim = _loss_args(kind, exclude, temperature, margin, hardest)
    if bias is not None:
        fn, sim = "szn_fused_simce_bias_head", sim + bias_args(kind, bias, K)
    if ws is None:
        buf = _scratch(nbytes, fmap.device)
    else:
        fn, buf = fn + "_prepared", ws.prepared(nbytes, emb, K, E, st)
    code = L.dtype_code(dmap.dtype) if dmap is not None else L.SZN_F32
    L.call(fn, stride, B, h, w, E, ld, 0, H, W, _CROP[stride], K, L.ptr(fmap), L.ptr(emb), L.ptr(target), classes, mode,
           L.ptr(gmap), *(sim + (L.ptr(loss), L.ptr(stats), L.ptr(pred), code, L.ptr(dmap), L.ptr(buf), st)))
    if ws is not None:
        ws.tables = Workspace.map_key(stride, fmap)


def embed_predict(kind, stride, fmap, emb, H, W, target=None, mode=0, unseen=None, gmap=None, exclude=None, temperature=None,
                  bias=None, margin=None, hardest=None):
    """forward-only embedding head -> (loss 0-dim tensor or None, pred (B,H,W) int64)"""
    B = fmap.shape[0]
    pred, tgt, loss = _outputs(B, H, W, fmap.device, target)
    stats = None if loss is None else torch.empty(B, 2, device=fmap.device)
    embed(kind, stride, fmap, emb, H, W, pred, tgt, loss, stats, mode=mode, classes=L.class_set(unseen), gmap=gmap, exclude=exclude,
          temperature=temperature, margin=margin, hardest=hardest, bias=bias)
    return (loss.reshape(()) if loss is not None else None), pred


def embed_loss(kind, stride, fmap, emb, H, W, target, exclude=None, temperature=None, ws=None, bias=None, margin=None, hardest=None):
    """the loss of embed_predict alone, bit for bit (the same kernels without the prediction: no trip through the classes per pixel)
    -> loss 0-dim tensor.  ws: a Workspace or None, as in embed()"""
    B = fmap.shape[0]
    tgt = target.to(device=fmap.device, dtype=torch.int64).contiguous()
    loss, stats = torch.empty(1, device=fmap.device), torch.empty(B, 2, device=fmap.device)
    embed(kind, stride, fmap, emb, H, W, None, tgt, loss, stats, ws=ws, exclude=exclude, temperature=temperature, margin=margin,
          hardest=hardest, bias=bias)
    return loss.reshape(())


def cosine(*args, **kw):
    """embed("cos", ...): the cosine loss (utils.cosine_loss)"""
    embed("cos", *args, **kw)


def cosine_predict(*args, **kw):
    return embed_predict("cos", *args, **kw)


def mse(*args, **kw):
    """embed("mse", ...): the MSE loss (utils.mse_loss) -- same arguments, same pred"""
    embed("mse", *args, **kw)


def mse_predict(*args, **kw):
    return embed_predict("mse", *args, **kw)


def sim_ce(*args, **kw):
    """embed("sim_ce", ...): the similarity cross-entropy loss (utils.sim_ce_loss) -- same arguments plus exclude / temperature, same pred"""
    embed("sim_ce", *args, **kw)


def sim_ce_predict(*args, **kw):
    return embed_predict("sim_ce", *args, **kw)


def sim_ce_bias(stride, fmap, emb, H, W, pred, unseen, weight, hidden=HIDDEN_LABEL, **kw):
    """embed("sim_ce", ..., bias=dict(unseen=, weight=, hidden=)): sim_ce plus the unseen-bias term on the pixels labelled `hidden`
    (utils.sim_ce_bias_loss) -- sim_ce's other arguments, same pred"""
    embed("sim_ce", stride, fmap, emb, H, W, pred, bias=dict(unseen=unseen, weight=weight, hidden=hidden), **kw)


def rank(*args, **kw):
    """embed("rank", ...): the hinge ranking loss (utils.rank_loss) -- same arguments plus exclude / margin / hardest, same pred"""
    embed("rank", *args, **kw)


def rank_predict(*args, **kw):
    return embed_predict("rank", *args, **kw)


# ---- view-ensemble embedding head (multi-scale / mirrored inference) ---------------------------------------------------------
def ms_views(H, W, scales, flip=False):
    """the views of an H x W input: [(Hs, Ws, flipped)] by ascending scale, the plain view before the mirrored one;
    Hs = max(1, floor(H * s + 0.5)).  `scales` must contain 1.0: the identity view's pass also gives the loss."""
    scales = sorted(float(s) for s in scales)
    if 1.0 not in scales:
        raise L.SznError("multi-scale inference: scales must contain 1.0 (got %r)" % (scales,))
    if any(not s > 0 for s in scales):
        raise L.SznError("multi-scale inference: scales must be positive (got %r)" % (scales,))
    views = []
    for s in scales:
        size = (max(1, int(H * s + 0.5)), max(1, int(W * s + 0.5)))
        views += [size + (False,)] + ([size + (True,)] if flip else [])
    if len(views) > L.MS_MAX_VIEWS:
        raise L.SznError("multi-scale inference: %d views, at most %d" % (len(views), L.MS_MAX_VIEWS))
    return views


def resize_flip(x, Hs, Ws, flip=False):
    """szn_resize_flip_f32: the (B,3,Hs,Ws) view of the (B,3,H,W) fp32 network input `x`, mirrored when `flip`"""
    x = x.to(torch.float32).contiguous()
    B, C, H, W = x.shape
    if C != 3:
        raise L.SznError("resize_flip: a (B,3,H,W) input is expected, got %r" % (tuple(x.shape),))
    out = torch.empty(B, 3, Hs, Ws, dtype=torch.float32, device=x.device)
    L.call("szn_resize_flip_f32", B, H, W, L.ptr(x), Hs, Ws, int(bool(flip)), L.ptr(out), L.stream_ptr())
    return out


def ms_predict(stride, views, emb, H, W, target=None, mode=0, unseen=None, gmap=None, want_acc=False):
    """szn_ms_head: views = [(fmap, Hs, Ws, flipped)], each fmap the contiguous fp32 NHWC map (the E embedding channels first) of the
    Hs x Ws view of one (B,3,H,W) batch, in ensemble order.  mode / unseen / gmap / target: the group rule of embed().
    -> pred (B,H,W) int64, or (pred, acc (B,H,W,K) fp32: the summed similarities before the group rule) with want_acc."""
    K, E = emb.shape
    if not views or len(views) > L.MS_MAX_VIEWS:
        raise L.SznError("ms_predict: %d views, between 1 and %d are taken" % (len(views), L.MS_MAX_VIEWS))
    B, dev = views[0][0].shape[0], views[0][0].device
    arr = (L.MsView * len(views))()
    for rec, (fmap, Hs, Ws, flipped) in zip(arr, views):
        if fmap.dtype != torch.float32 or not fmap.is_contiguous() or fmap.dim() != 4 or fmap.shape[0] != B:
            raise L.SznError("ms_predict: every view's map must be a contiguous fp32 (B,h,w,C) tensor")
        rec.coarse, rec.h, rec.w, rec.ldc, rec.c0 = fmap.data_ptr(), fmap.shape[1], fmap.shape[2], fmap.shape[3], 0
        rec.Hs, rec.Ws, rec.flip = int(Hs), int(Ws), int(bool(flipped))
    nbytes = L.load().szn_ms_head_workspace_bytes(stride, B, E, K, len(views), arr)
    if nbytes == 0:
        raise L.SznError("ms_predict: bad geometry (stride %d, B %d, E %d, K %d, %d views)" % (stride, B, E, K, len(views)))
    buf = _scratch(nbytes, dev)
    pred = torch.empty(B, H, W, dtype=torch.int64, device=dev)
    acc = torch.empty(B, H, W, K, dtype=torch.float32, device=dev) if want_acc else None
    tgt = None if target is None else target.to(device=dev, dtype=torch.int64).contiguous()
    L.call("szn_ms_head", stride, B, E, K, H, W, _CROP[stride], len(views), arr, L.ptr(emb), L.class_set(unseen), mode, L.ptr(gmap),
           L.ptr(tgt), L.ptr(pred), L.ptr(acc), L.ptr(buf), L.stream_ptr())
    return (pred, acc) if want_acc else pred


# ---- calibrated stacking: seen-class penalty, one-pass sweep -----------------------------------------------------------------
def _sweep_values(who, noun, values, most):
    """the candidate values of a sweep as the float32 HOST array the sweep heads read: 1 to `most` finite, strictly ascending values"""
    import numpy as np
    v = np.ascontiguousarray(np.asarray(values, dtype=np.float32).reshape(-1))
    if not 1 <= v.size <= most:
        raise L.SznError("%s: %d %s, between 1 and %d are taken" % (who, v.size, noun, most))
    if not np.isfinite(v).all() or not (np.diff(v) > 0).all():
        raise L.SznError("%s: the %s must be finite and strictly ascending as float32 (got %r)" % (who, noun, v.tolist()))
    return v


def calib_gammas(gammas):
    """the candidate penalties as the float32 HOST array szn_calib_head reads: 1 to CALIB_MAX_GAMMAS finite, strictly ascending values"""
    return _sweep_values("calibration", "gammas", gammas, L.CALIB_MAX_GAMMAS)


def _check_map(who, fmap):
    if fmap.dtype != torch.float32 or not fmap.is_contiguous():
        raise L.SznError("%s: the map must be a contiguous fp32 (B,h,w,C) tensor" % who)


class _SweepCall(object):
    """the host front end calib, hub, conse, seen_sweep and soft_gate share, after the map check and their own checks: the values
    (`noun` "gammas": calib_gammas, "taus": seen_sweep_taus), then what target / hist / pred_index ask for.  extra: None, or (name,
    wanted) of a further output that counts as something to compute.  Holds what the C side takes: tgt (the target as int64 on the
    map's device, or None), hist, pred (an empty (B,H,W) int64 tensor, or None without a pred_index), G, values (the host float
    pointer) and pred_index (-1: none)."""

    def __init__(self, who, noun, fmap, emb, H, W, values, target, hist, pred_index, extra=None):
        import ctypes as C
        v = (calib_gammas if noun == "gammas" else seen_sweep_taus)(values)
        G, K, dev = int(v.size), emb.shape[0], fmap.device
        if target is None and hist is not None:
            raise L.SznError("%s: a histogram needs the target" % who)
        if target is None and pred_index is None and not (extra and extra[1]):
            raise L.SznError("%s: nothing to compute (no target for a histogram, no pred_index for a prediction%s)"
                             % (who, ", no " + extra[0] if extra else ""))
        if pred_index is not None and not 0 <= int(pred_index) < G:
            raise L.SznError("%s: pred_index %r outside [0, %d)" % (who, pred_index, G))
        self.tgt = None
        if target is not None:
            self.tgt = target.to(device=dev, dtype=torch.int64).contiguous()
            if hist is None:
                hist = torch.zeros(G, K, K, dtype=torch.int64, device=dev)
            elif hist.dtype != torch.int64 or tuple(hist.shape) != (G, K, K) or not hist.is_contiguous() or hist.device != dev:
                raise L.SznError("%s: hist must be a contiguous int64 (%d,%d,%d) tensor on %s" % (who, G, K, K, dev))
        self.who, self.noun, self.fmap, self.emb, self.hist, self.G = who, noun, fmap, emb, hist, G
        self.pred = torch.empty(fmap.shape[0], H, W, dtype=torch.int64, device=dev) if pred_index is not None else None
        self.values = v.ctypes.data_as(C.POINTER(C.c_float))       # (the pointer object keeps the array alive)
        self.pred_index = -1 if pred_index is None else int(pred_index)

    def scratch(self, stride, nbytes, ws=None):
        """the head's workspace from what its szn_*_workspace_bytes said (0: a geometry it refuses): fresh scratch, or the buffer of
        the Workspace `ws` when that holds this map's tables (Workspace.holds)"""
        B, h, w, _ = self.fmap.shape
        K, E = self.emb.shape
        if nbytes == 0:
            raise L.SznError("%s: bad geometry (stride %d, B %d, map %d x %d, E %d, K %d, %d %s)"
                             % (self.who, stride, B, h, w, E, K, self.G, self.noun))
        if ws is None:
            return _scratch(nbytes, self.fmap.device)
        if not ws.holds(nbytes, stride, self.fmap, self.emb):
            raise L.SznError("%s: ws must be the Workspace in which the embedding head last ran on this very map and embedding "
                             "matrix, %d bytes or more" % (self.who, nbytes))
        return ws.buf


def calib(stride, fmap, emb, H, W, unseen, gammas, target=None, hist=None, pred_index=None):
    """szn_calib_head on the contiguous fp32 NHWC map `fmap` (the E embedding channels first): gamma is subtracted from the
    similarity of every class NOT in `unseen` before the argmax, for every gamma of `gammas` (ascending) in one pass.
    target given: hist (G,K,K) int64 += the confusion counts of every gamma (allocated as zeros when None).  pred_index given: pred
    (B,H,W) int64 at gammas[pred_index].  -> (hist or None, pred or None)"""
    B, h, w, ld = fmap.shape
    K, E = emb.shape
    _check_map("calib", fmap)
    s = _SweepCall("calib", "gammas", fmap, emb, H, W, gammas, target, hist, pred_index)
    buf = s.scratch(stride, L.load().szn_calib_head_workspace_bytes(stride, B, h, w, E, K, s.G))
    L.call("szn_calib_head", stride, B, h, w, E, ld, 0, H, W, _CROP[stride], K, L.ptr(fmap), L.ptr(emb), L.ptr(s.tgt),
           L.class_set(unseen), s.G, s.values, L.ptr(s.hist), s.pred_index, L.ptr(s.pred), L.ptr(buf), L.stream_ptr())
    return s.hist, s.pred


# ---- hubness correction: per-image, per-class centering / standardising of the similarities ----------------------------------------
HUB_BETA = 1.0           # the textbook form (the whole mean is subtracted); a default nobody has tuned
HUB_MIN_SD = 0.05        # floor of the standard deviation in zscore mode; a default nobody has tuned


def hub_params(cfg):
    """a hubness-correction description dict(mode=, beta=, min_sd=) checked -> dict(mode=, beta=, min_sd=) with the float32 values
    szn_hub_stats reads: mode 'mean' | 'zscore' (required), beta finite and >= 0 (None or absent: HUB_BETA), min_sd finite and > 0
    (None or absent: HUB_MIN_SD)"""
    import numpy as np
    if not isinstance(cfg, dict) or set(cfg) - {"mode", "beta", "min_sd"} or cfg.get("mode") not in L.HUB_MODES:
        raise L.SznError("hub: the correction must be dict(mode='mean' | 'zscore', beta=, min_sd=), got %r" % (cfg,))
    beta, min_sd = cfg.get("beta"), cfg.get("min_sd")
    try:
        b = float(np.float32(HUB_BETA if beta is None else beta))
        s = float(np.float32(HUB_MIN_SD if min_sd is None else min_sd))
    except (TypeError, ValueError):
        raise L.SznError("hub: beta and min_sd must be numbers, got %r" % (cfg,))
    if not np.isfinite(b) or b < 0:
        raise L.SznError("hub: beta must be finite and >= 0 (got %r)" % (beta,))
    if not np.isfinite(s) or s <= 0:
        raise L.SznError("hub: min_sd must be finite and > 0 (got %r)" % (min_sd,))
    return dict(mode=cfg["mode"], beta=b, min_sd=s)


def hub_stats(stride, fmap, emb, H, W, mode, beta, min_sd, target=None, want=()):
    """szn_hub_stats on the contiguous fp32 NHWC map `fmap` (the E embedding channels first): per image and class the (scale, shift) pair
    of the hubness correction, from the exact int64 moments of the class's similarity over the image's pixels (those `target` labels
    PAD_LABEL and zero-norm pixels left out).  want: any of 'sums' ((B,K,2) int64: S1, S2 in units of 2^-20 / 2^-40) and 'counts' ((B,)
    int64).  -> table (B,K,2) fp32, or (table, *requested) in the order of `want`.  No host synchronisation."""
    B, h, w, ld = fmap.shape
    K, E = emb.shape
    if fmap.dtype != torch.float32 or not fmap.is_contiguous():
        raise L.SznError("hub_stats: the map must be a contiguous fp32 (B,h,w,C) tensor")
    p = hub_params(dict(mode=mode, beta=beta, min_sd=min_sd))
    want = tuple(want)
    if set(want) - {"sums", "counts"}:
        raise L.SznError("hub_stats: want holds 'sums' and / or 'counts', got %r" % (want,))
    dev = fmap.device
    tgt = None if target is None else target.to(device=dev, dtype=torch.int64).contiguous()
    table = torch.empty(B, K, 2, dtype=torch.float32, device=dev)
    extra = {"sums": torch.empty(B, K, 2, dtype=torch.int64, device=dev) if "sums" in want else None,
             "counts": torch.empty(B, dtype=torch.int64, device=dev) if "counts" in want else None}
    nbytes = L.load().szn_hub_stats_workspace_bytes(stride, B, h, w, E, K)
    if nbytes == 0:
        raise L.SznError("hub_stats: bad geometry (stride %d, B %d, map %d x %d, E %d, K %d)" % (stride, B, h, w, E, K))
    buf = _scratch(nbytes, dev)
    L.call("szn_hub_stats", stride, B, h, w, E, ld, 0, H, W, _CROP[stride], K, L.ptr(fmap), L.ptr(emb), L.ptr(tgt), L.HUB_MODES[p["mode"]],
           p["beta"], p["min_sd"], L.ptr(table), L.ptr(extra["sums"]), L.ptr(extra["counts"]), L.ptr(buf), L.stream_ptr())
    return (table,) + tuple(extra[k] for k in want) if want else table


def hub(stride, fmap, emb, H, W, unseen, table, gammas, target=None, hist=None, pred_index=None):
    """szn_hub_head: calib() on the corrected similarities fmaf(sim, table[b][k][0], -table[b][k][1]) -- table (B,K,2) fp32 from hub_stats, or
    the caller's own.  Everything else is calib()'s: the gammas, hist, pred_index, what comes back.  -> (hist or None, pred or None)"""
    B, h, w, ld = fmap.shape
    K, E = emb.shape
    _check_map("hub", fmap)
    dev = fmap.device
    if (not isinstance(table, torch.Tensor) or table.dtype != torch.float32 or tuple(table.shape) != (B, K, 2) or not table.is_contiguous()
            or table.device != dev):
        raise L.SznError("hub: table must be a contiguous fp32 (%d,%d,2) tensor on %s" % (B, K, dev))
    s = _SweepCall("hub", "gammas", fmap, emb, H, W, gammas, target, hist, pred_index)
    buf = s.scratch(stride, L.load().szn_hub_head_workspace_bytes(stride, B, h, w, E, K, s.G))
    L.call("szn_hub_head", stride, B, h, w, E, ld, 0, H, W, _CROP[stride], K, L.ptr(fmap), L.ptr(emb), L.ptr(s.tgt), L.class_set(unseen),
           L.ptr(table), s.G, s.values, L.ptr(s.hist), s.pred_index, L.ptr(s.pred), L.ptr(buf), L.stream_ptr())
    return s.hist, s.pred


# ---- ConSE: zero-shot inference for the softmax FCN ---------------------------------------------------------------------------
def conse_top(top_t):
    """ConSE's T as szn_conse_head takes it: an integer in [1, CONSE_MAX_TOP]"""
    if isinstance(top_t, bool) or int(top_t) != top_t or not 1 <= int(top_t) <= L.CONSE_MAX_TOP:
        raise L.SznError("conse: top_t must be an integer in [1, %d], got %r" % (L.CONSE_MAX_TOP, top_t))
    return int(top_t)


def conse(stride, fmap, emb, H, W, unseen, top_t, gammas=None, target=None, hist=None, pred_index=None, forced=False):
    """szn_conse_head on the contiguous fp32 NHWC LOGIT map `fmap` of a softmax network (the K class channels first) with the (K,E)
    class embeddings `emb`: per pixel the softmax over the classes NOT in `unseen`, its top `top_t`, the probability-weighted mean of
    their embeddings, and the nearest class by cosine among all classes, with calib()'s penalty gamma on the seen classes -- for
    every gamma of `gammas` (ascending) in one pass.  target given: hist (G,K,K) int64 += the confusion counts of every gamma
    (allocated as zeros when None).  pred_index given: pred (B,H,W) int64 at gammas[pred_index].  forced=True (the reference's -fu):
    pred = the best unseen class where `target` names an unseen class, the best seen class elsewhere; no gammas, no hist.
    -> (hist or None, pred or None)"""
    B, h, w, ld = fmap.shape
    K, E = emb.shape
    _check_map("conse", fmap)
    if emb.dtype != torch.float32 or not emb.is_contiguous() or emb.device != fmap.device:
        raise L.SznError("conse: the embeddings must be a contiguous fp32 (K,E) tensor on the map's device")
    top_t = conse_top(top_t)
    dev = fmap.device
    tgt = None if target is None else target.to(device=dev, dtype=torch.int64).contiguous()
    if forced:
        if gammas is not None or hist is not None or pred_index is not None:
            raise L.SznError("conse: a forced call takes no gammas, hist or pred_index")
        if tgt is None:
            raise L.SznError("conse: a forced call needs the target")
        G, gp, pidx = 0, None, 0
        pred = torch.empty(B, H, W, dtype=torch.int64, device=dev)
    else:
        if gammas is None:
            raise L.SznError("conse: gammas are required (forced=False)")
        s = _SweepCall("conse", "gammas", fmap, emb, H, W, gammas, tgt, hist, pred_index)
        G, gp, hist, pidx, pred = s.G, s.values, s.hist, s.pred_index, s.pred
    nbytes = L.load().szn_conse_head_workspace_bytes(stride, B, h, w, E, K, G)
    if nbytes == 0:         # (both branches: a forced call has no sweep to ask)
        raise L.SznError("conse: bad geometry (stride %d, B %d, map %d x %d, E %d, K %d, %d gammas)" % (stride, B, h, w, E, K, G))
    buf = _scratch(nbytes, dev)
    L.call("szn_conse_head", stride, B, h, w, K, ld, 0, H, W, _CROP[stride], E, L.ptr(fmap), L.ptr(emb), L.ptr(tgt),
           L.class_set(unseen), top_t, int(bool(forced)), G, gp, L.ptr(hist), pidx, L.ptr(pred), L.ptr(buf), L.stream_ptr())
    return hist, pred


# ---- full SZN inference with a seen-mask threshold: one-pass sweep ---------------------------------------------------------------
def seen_sweep_taus(taus):
    """the candidate thresholds (logit units) as the float32 HOST array szn_seen_sweep_head reads: 1 to SEEN_SWEEP_MAX_TAUS finite,
    strictly ascending values"""
    return _sweep_values("seen sweep", "taus", taus, L.SEEN_SWEEP_MAX_TAUS)


def seen_sweep_workspace_bytes(stride, fmap, emb, n_taus):
    """szn_seen_sweep_head_workspace_bytes for a map and an embedding matrix (0: a geometry the head refuses)"""
    B, h, w, _ = fmap.shape
    K, E = emb.shape
    return L.load().szn_seen_sweep_head_workspace_bytes(stride, B, h, w, E, K, int(n_taus))


def _check_margin(who, margin, B, H, W, dev):
    if margin is None or margin.dtype != torch.float32 or tuple(margin.shape) != (B, H, W) or not margin.is_contiguous() or margin.device != dev:
        raise L.SznError("%s: margin must be a contiguous fp32 (%d,%d,%d) tensor on %s" % (who, B, H, W, dev))


def seen_sweep(stride, fmap, emb, H, W, unseen, margin, taus, target=None, hist=None, pred_index=None, ws=None):
    """szn_seen_sweep_head on the contiguous fp32 NHWC map `fmap` (the E embedding channels first): the grouped head's class assignment
    with a pixel in the seen group iff margin > tau (margin: seenmask_margin's (B,H,W) f32 map), for every tau of `taus` (ascending) in
    one pass.  target given: hist (G,K,K) int64 += the confusion counts of every tau (allocated as zeros when None).  pred_index given:
    pred (B,H,W) int64 at taus[pred_index].  -> (hist or None, pred or None).  ws: None, or the Workspace in which embed() / embed_loss()
    has just run on this very map and embedding matrix, already as large as seen_sweep_workspace_bytes says: the embedding tables and the
    stride-8 position tables that call left there are reused (szn_seen_sweep_head_tabled)"""
    B, h, w, ld = fmap.shape
    K, E = emb.shape
    _check_map("seen_sweep", fmap)
    _check_margin("seen_sweep", margin, B, H, W, fmap.device)
    s = _SweepCall("seen_sweep", "taus", fmap, emb, H, W, taus, target, hist, pred_index)
    buf = s.scratch(stride, seen_sweep_workspace_bytes(stride, fmap, emb, s.G), ws)
    L.call("szn_seen_sweep_head" if ws is None else "szn_seen_sweep_head_tabled", stride, B, h, w, E, ld, 0, H, W, _CROP[stride], K,
           L.ptr(fmap), L.ptr(emb), L.ptr(s.tgt), L.class_set(unseen), L.ptr(margin), s.G, s.values, L.ptr(s.hist), s.pred_index,
           L.ptr(s.pred), L.ptr(buf), L.stream_ptr())
    return s.hist, s.pred


# ---- full SZN inference with a soft seen/unseen gate ----------------------------------------------------------------------------
GATE_TEMPERATURE = 0.1       # the default of train.py --gate-temperature: a hyper-parameter default, not a tuned value


def gate_params(gate):
    """a gate description dict(weight=, temperature=) checked -> (weight, temperature) as the float32 values szn_soft_gate_head reads:
    weight finite and >= 0 (required), temperature finite and > 0 (None or absent: GATE_TEMPERATURE)"""
    import numpy as np
    if not isinstance(gate, dict) or set(gate) - {"weight", "temperature"} or "weight" not in gate:
        raise L.SznError("soft gate: gate must be dict(weight=, temperature=) with a weight, got %r" % (gate,))
    temperature = gate.get("temperature")
    try:
        w = float(np.float32(gate["weight"]))
        t = float(np.float32(GATE_TEMPERATURE if temperature is None else temperature))
    except (TypeError, ValueError):
        raise L.SznError("soft gate: weight and temperature must be numbers, got %r" % (gate,))
    if not np.isfinite(w) or w < 0:
        raise L.SznError("soft gate: weight must be finite and >= 0 (got %r)" % (gate["weight"],))
    if not np.isfinite(t) or t <= 0:
        raise L.SznError("soft gate: temperature must be finite and > 0 (got %r)" % (temperature,))
    return w, t


def soft_gate_workspace_bytes(stride, fmap, emb, n_taus):
    """szn_soft_gate_head_workspace_bytes for a map and an embedding matrix (0: a geometry the head refuses)"""
    B, h, w, _ = fmap.shape
    K, E = emb.shape
    return L.load().szn_soft_gate_head_workspace_bytes(stride, B, h, w, E, K, int(n_taus))


def soft_gate(stride, fmap, emb, H, W, unseen, margin, taus, temperature, weight, target=None, hist=None, pred_index=None,
              want_eff=False, ws=None):
    """szn_soft_gate_head on the contiguous fp32 NHWC map `fmap` (the E embedding channels first): seen_sweep() with the probabilistic
    gate p(k|x) = p(group|x) p(k|group,x) -- a pixel takes its best seen class iff e = margin - weight * (l_S - l_U) > tau, l_G = -log of
    the best class's softmax probability inside its group at `temperature`, and its best unseen class otherwise; the two candidates are
    the true in-group argmaxes.  Every tau of `taus` (ascending) in one pass.  target given: hist (G,K,K) int64 += the confusion counts of
    every tau (allocated as zeros when None).  pred_index given: pred (B,H,W) int64 at taus[pred_index].  want_eff: eff (B,H,W) f32 = e.
    -> (hist or None, pred or None, eff or None).  ws: as in seen_sweep() (szn_soft_gate_head_tabled)"""
    B, h, w, ld = fmap.shape
    K, E = emb.shape
    _check_map("soft_gate", fmap)
    _check_margin("soft_gate", margin, B, H, W, fmap.device)
    wgt, temp = gate_params(dict(weight=weight, temperature=temperature))
    s = _SweepCall("soft_gate", "taus", fmap, emb, H, W, taus, target, hist, pred_index, extra=("eff", want_eff))
    eff = torch.empty(B, H, W, dtype=torch.float32, device=fmap.device) if want_eff else None
    buf = s.scratch(stride, soft_gate_workspace_bytes(stride, fmap, emb, s.G), ws)
    L.call("szn_soft_gate_head" if ws is None else "szn_soft_gate_head_tabled", stride, B, h, w, E, ld, 0, H, W, _CROP[stride], K,
           L.ptr(fmap), L.ptr(emb), L.ptr(s.tgt), L.class_set(unseen), L.ptr(margin), temp, wgt, s.G, s.values, L.ptr(s.hist),
           s.pred_index, L.ptr(s.pred), L.ptr(eff), L.ptr(buf), L.stream_ptr())
    return s.hist, s.pred, eff


# ---- self-training: top-p% pseudo labels on the hidden pixels ------------------------------------------------------------------
_PSEUDO_EXTRAS = ("cand", "conf", "qhist", "thr", "counts")


def _permille(who, keep):
    """a share in (0, 1] as the integer permille szn_pseudo_head / szn_ohem_head take (rounded; at least 1)"""
    try:
        k = float(keep)
    except (TypeError, ValueError):
        raise L.SznError("%s: keep must be a number in (0, 1], got %r" % (who, keep))
    if not 0.0 < k <= 1.0:
        raise L.SznError("%s: keep must lie in (0, 1], got %r" % (who, keep))
    return max(1, int(round(k * 1000.0)))


def pseudo_permille(keep):
    """the share of the candidates to keep, a number in (0, 1], as the integer permille szn_pseudo_head takes (rounded; at least 1)"""
    return _permille("pseudo labels", keep)


def pseudo_call(stride, fmap, emb, H, W, target, unseen_cs, gamma, permille, conf_floor, cand_label, target_out, ws_buf, stream,
                cand=None, conf=None, qhist=None, thr=None, counts=None):
    """szn_pseudo_head with every buffer supplied by the caller (engine.TrainStep: no allocation on the step path)"""
    B, h, w, ld = fmap.shape
    K, E = emb.shape
    L.call("szn_pseudo_head", stride, B, h, w, E, ld, 0, H, W, _CROP[stride], K, L.ptr(fmap), L.ptr(emb), L.ptr(target), unseen_cs,
           float(gamma), float(conf_floor), int(permille), int(cand_label), L.ptr(target_out), L.ptr(cand), L.ptr(conf), L.ptr(qhist),
           L.ptr(thr), L.ptr(counts), L.ptr(ws_buf), stream)


def pseudo_workspace_bytes(stride, fmap, emb, H, W):
    B, h, w, _ = fmap.shape
    K, E = emb.shape
    nbytes = L.load().szn_pseudo_head_workspace_bytes(stride, B, h, w, E, K, H, W)
    if nbytes == 0:
        raise L.SznError("pseudo: bad geometry (stride %d, B %d, map %d x %d, E %d, K %d, image %d x %d)" % (stride, B, h, w, E, K, H, W))
    return nbytes


def pseudo(stride, fmap, emb, H, W, target, unseen, gamma=0.0, keep=0.3, conf_floor=-2.0, cand_label=HIDDEN_LABEL, want=()):
    """szn_pseudo_head on the contiguous fp32 NHWC map `fmap` (the E embedding channels first): among the pixels whose target is
    cand_label, those the calibrated rule at `gamma` gives to an unseen class with a similarity of at least conf_floor are candidates;
    per unseen class the most confident `keep` of them (whole confidence bins of 1/512) take that class as their label.
    -> target_out (B,H,W) int64, or (target_out, {name: tensor}) with want = names among cand, conf, qhist, thr, counts."""
    import math
    K, E = emb.shape
    B = fmap.shape[0]
    if fmap.dtype != torch.float32 or not fmap.is_contiguous() or fmap.dim() != 4:
        raise L.SznError("pseudo: the map must be a contiguous fp32 (B,h,w,C) tensor")
    permille = pseudo_permille(keep)
    if not (math.isfinite(float(gamma)) and math.isfinite(float(conf_floor))):
        raise L.SznError("pseudo: gamma and conf_floor must be finite (got %r, %r)" % (gamma, conf_floor))
    if int(cand_label) >= 0:
        raise L.SznError("pseudo: cand_label must be negative (got %r): a class label cannot mark the hidden pixels" % (cand_label,))
    want = (want,) if isinstance(want, str) else tuple(want)
    bad = [n for n in want if n not in _PSEUDO_EXTRAS]
    if bad:
        raise L.SznError("pseudo: want names %r; known: %s" % (bad, ", ".join(_PSEUDO_EXTRAS)))
    if target is None:
        raise L.SznError("pseudo: the target is required")
    dev = fmap.device
    tgt = target.to(device=dev, dtype=torch.int64).contiguous()
    if tuple(tgt.shape) != (B, H, W):
        raise L.SznError("pseudo: target shape %r, expected %r" % (tuple(tgt.shape), (B, H, W)))
    out = torch.empty(B, H, W, dtype=torch.int64, device=dev)
    shapes = dict(cand=((B, H, W), torch.int64), conf=((B, H, W), torch.float32), qhist=((K, L.PSEUDO_BINS), torch.int64),
                  thr=((K,), torch.int32), counts=((K, 2), torch.int64))
    extra = {n: torch.empty(shapes[n][0], dtype=shapes[n][1], device=dev) for n in want}
    buf = _scratch(pseudo_workspace_bytes(stride, fmap, emb, H, W), dev)
    pseudo_call(stride, fmap, emb, H, W, tgt, L.class_set(unseen), gamma, permille, conf_floor, cand_label, out, buf, L.stream_ptr(),
                **extra)
    return (out, extra) if want else out


# ---- hard-pixel mining: keep the hardest labelled pixels of every image -----------------------------------------------------------
OHEM_DROP_LABEL = -1        # the label a mined-out pixel reads: every loss and metric kernel ignores it
_OHEM_EXTRAS = ("conf", "qhist", "cut", "counts")


def ohem_permille(keep):
    """the share of an image's labelled pixels to keep, a number in (0, 1], as the integer permille szn_ohem_head takes (rounded; at
    least 1)"""
    return _permille("ohem", keep)


def ohem_call(stride, fmap, emb, H, W, target, skip_cs, permille, thresh, drop_label, target_out, ws_buf, stream, conf=None, qhist=None,
              cut=None, counts=None):
    """szn_ohem_head with every buffer supplied by the caller (engine.TrainStep: no allocation on the step path); skip_cs: a
    _lib.class_set or None"""
    B, h, w, ld = fmap.shape
    K, E = emb.shape
    L.call("szn_ohem_head", stride, B, h, w, E, ld, 0, H, W, _CROP[stride], K, L.ptr(fmap), L.ptr(emb), L.ptr(target), skip_cs,
           int(permille), float(thresh), int(drop_label), L.ptr(target_out), L.ptr(conf), L.ptr(qhist), L.ptr(cut), L.ptr(counts),
           L.ptr(ws_buf), stream)


def ohem_workspace_bytes(stride, fmap, emb, H, W):
    B, h, w, _ = fmap.shape
    K, E = emb.shape
    nbytes = L.load().szn_ohem_head_workspace_bytes(stride, B, h, w, E, K, H, W)
    if nbytes == 0:
        raise L.SznError("ohem: bad geometry (stride %d, B %d, map %d x %d, E %d, K %d, image %d x %d)" % (stride, B, h, w, E, K, H, W))
    return nbytes


def ohem(stride, fmap, emb, H, W, target, keep, thresh=None, skip=None, drop_label=OHEM_DROP_LABEL, want=()):
    """szn_ohem_head on the contiguous fp32 NHWC map `fmap` (the E embedding channels first): per image the `keep` of the labelled
    pixels (label in [0, K), not in `skip`) whose cosine to their own class embedding is lowest, and every pixel whose cosine lies below
    `thresh` (None: no threshold; rounded down to a multiple of 1/512), keep their label; the others read drop_label.
    -> target_out (B,H,W) int64, or (target_out, {name: tensor}) with want = names among conf, qhist, cut, counts."""
    import math
    K, E = emb.shape
    B = fmap.shape[0]
    if fmap.dtype != torch.float32 or not fmap.is_contiguous() or fmap.dim() != 4:
        raise L.SznError("ohem: the map must be a contiguous fp32 (B,h,w,C) tensor")
    permille = ohem_permille(keep)
    thresh = -2.0 if thresh is None else float(thresh)
    if not math.isfinite(thresh):
        raise L.SznError("ohem: thresh must be finite or None (got %r)" % (thresh,))
    if int(drop_label) >= 0:
        raise L.SznError("ohem: drop_label must be negative (got %r): a class label cannot mark the dropped pixels" % (drop_label,))
    skip = sorted(set(int(k) for k in (skip or ())))
    if skip and (skip[0] < 0 or skip[-1] >= K or len(skip) >= K):
        raise L.SznError("ohem: skip must name some, not all, classes of [0, %d) (got %r)" % (K, skip))
    want = (want,) if isinstance(want, str) else tuple(want)
    bad = [n for n in want if n not in _OHEM_EXTRAS]
    if bad:
        raise L.SznError("ohem: want names %r; known: %s" % (bad, ", ".join(_OHEM_EXTRAS)))
    if target is None:
        raise L.SznError("ohem: the target is required")
    dev = fmap.device
    tgt = target.to(device=dev, dtype=torch.int64).contiguous()
    if tuple(tgt.shape) != (B, H, W):
        raise L.SznError("ohem: target shape %r, expected %r" % (tuple(tgt.shape), (B, H, W)))
    out = torch.empty(B, H, W, dtype=torch.int64, device=dev)
    shapes = dict(conf=((B, H, W), torch.float32), qhist=((B, L.OHEM_BINS), torch.int64), cut=((B,), torch.int32),
                  counts=((B, 2), torch.int64))
    extra = {n: torch.empty(shapes[n][0], dtype=shapes[n][1], device=dev) for n in want}
    buf = _scratch(ohem_workspace_bytes(stride, fmap, emb, H, W), dev)
    ohem_call(stride, fmap, emb, H, W, tgt, L.class_set(skip) if skip else None, permille, thresh, drop_label, out, buf, L.stream_ptr(),
              **extra)
    return (out, extra) if want else out


# ---- class prototypes: masked average pooling of the upsampled score ------------------------------------------------------------
_PROTO_MODE = {"raw": L.PROTO_RAW, "unit": L.PROTO_UNIT}


def proto_mode(mode):
    """"unit" | "raw" -> szn_class_proto's mode argument"""
    if mode not in _PROTO_MODE:
        raise L.SznError("class_proto: mode must be 'unit' or 'raw', got %r" % (mode,))
    return _PROTO_MODE[mode]


def proto_workspace_bytes(stride, fmap, E, K):
    B, h, w, _ = fmap.shape
    nbytes = L.load().szn_class_proto_workspace_bytes(stride, B, h, w, E, K)
    if nbytes == 0:
        raise L.SznError("class_proto: bad geometry (stride %d, B %d, map %d x %d, E %d, K %d)" % (stride, B, h, w, E, K))
    return nbytes


def proto_call(stride, fmap, E, H, W, labels, K, classes_cs, mode_code, accumulate, sums, counts, ws_buf, stream):
    """szn_class_proto with every buffer supplied by the caller; classes_cs: a _lib.class_set or None (all K classes)"""
    B, h, w, ld = fmap.shape
    L.call("szn_class_proto", stride, B, h, w, E, ld, 0, H, W, _CROP[stride], K, L.ptr(fmap), L.ptr(labels), classes_cs, int(mode_code),
           int(accumulate), L.ptr(sums), L.ptr(counts), L.ptr(ws_buf), stream)


def class_proto(stride, fmap, H, W, labels, K, classes=None, mode="unit", out=None, E=None):
    """szn_class_proto on the contiguous fp32 NHWC map `fmap` (the E embedding channels first; E: None = all its channels): per class k
    of `classes` (None: all K) the sum over the pixels labelled k of the upsampled score's unit vector (mode "unit") or of the score
    itself ("raw"), and the pixel counts {labelled, summed}.  labels: any (B,H,W) integer map; every label outside [0, K) or outside
    `classes` is skipped.  out = (sums, counts) of an earlier call: this call's values are added to them (a support set pooled batch by
    batch).  -> (sums (K,E) float64, counts (K,2) int64) on the map's device."""
    if fmap.dtype != torch.float32 or not fmap.is_contiguous() or fmap.dim() != 4:
        raise L.SznError("class_proto: the map must be a contiguous fp32 (B,h,w,C) tensor")
    B, _, _, ld = fmap.shape
    E = ld if E is None else int(E)
    K = int(K)
    code = proto_mode(mode)
    if not 1 <= E <= ld:
        raise L.SznError("class_proto: E = %d outside [1, %d], the map's channels" % (E, ld))
    if not 1 <= K <= L.MAX_CLASSES:
        raise L.SznError("class_proto: K = %d outside [1, %d]" % (K, L.MAX_CLASSES))
    cs = None
    if classes is not None:
        classes = sorted(set(int(k) for k in classes))
        if not classes or classes[0] < 0 or classes[-1] >= K:
            raise L.SznError("class_proto: classes must name at least one class of [0, %d) (got %r)" % (K, classes))
        cs = L.class_set(classes)
    if labels is None:
        raise L.SznError("class_proto: the label map is required")
    dev = fmap.device
    lbl = labels.to(device=dev, dtype=torch.int64).contiguous()
    if tuple(lbl.shape) != (B, H, W):
        raise L.SznError("class_proto: labels shape %r, expected %r" % (tuple(lbl.shape), (B, H, W)))
    if out is None:
        sums = torch.empty(K, E, dtype=torch.float64, device=dev)
        counts = torch.empty(K, 2, dtype=torch.int64, device=dev)
    else:
        sums, counts = out
        if (sums.dtype != torch.float64 or tuple(sums.shape) != (K, E) or not sums.is_contiguous() or sums.device != dev
                or counts.dtype != torch.int64 or tuple(counts.shape) != (K, 2) or not counts.is_contiguous() or counts.device != dev):
            raise L.SznError("class_proto: out must be (float64 (%d,%d), int64 (%d,2)) contiguous tensors on %s" % (K, E, K, dev))
    buf = _scratch(proto_workspace_bytes(stride, fmap, E, K), dev)
    proto_call(stride, fmap, E, H, W, lbl, K, cs, code, out is not None, sums, counts, buf, L.stream_ptr())
    return sums, counts


# ---- softmax cross-entropy head -------------------------------------------------------------------------------------------
def ce(stride, fmap, C, H, W, pred, target=None, weight=None, size_average=False, loss=None, stats=None, dmap=None, ws=None,
       stream=None):
    """szn_fused_ce_head on the contiguous NHWC map `fmap` (the C class channels first); arguments as in cosine()"""
    B, h, w, ld = fmap.shape
    nbytes = L.load().szn_fused_ce_head_workspace_bytes(stride, B, h, w, C)
    buf = _scratch(nbytes, fmap.device) if ws is None else ws.get(nbytes)
    code = L.dtype_code(dmap.dtype) if dmap is not None else L.SZN_F32
    L.call("szn_fused_ce_head", stride, B, h, w, C, ld, 0, H, W, _CROP[stride], L.ptr(fmap), L.ptr(target), L.ptr(weight),
           int(size_average), L.ptr(loss), L.ptr(stats), L.ptr(pred), code, L.ptr(dmap), L.ptr(buf),
           L.stream_ptr() if stream is None else stream)


def ce_predict(stride, fmap, C, H, W, target=None, weight=None):
    """forward-only softmax head (summed cross entropy, optional class weights) -> (loss 0-dim tensor or None, pred)"""
    if C > L.MAX_CLASSES:
        raise L.SznError("softmax_predict: the fused head holds at most %d classes, got %d" % (L.MAX_CLASSES, C))
    pred, tgt, loss = _outputs(fmap.shape[0], H, W, fmap.device, target)
    wt = None
    if target is not None and weight is not None:
        wt = torch.as_tensor(weight).to(fmap.device, torch.float32).contiguous()
        if wt.numel() != C:
            raise L.SznError("softmax_predict: weight has %d entries for %d classes" % (wt.numel(), C))
    ce(stride, fmap, C, H, W, pred, tgt, wt, loss=loss)
    return (loss.reshape(()) if loss is not None else None), pred


# ---- x32 seen-mask head ---------------------------------------------------------------------------------------------------
def seenmask(coarse, E, up_w, pred, target=None, n_class=0, seen=None, loss=None, stats=None, conf=None, dscore=None, dup_w=None,
             ws=None, stream=None):
    """szn_seenmask_head_k on the 1/32 map `coarse` (B,h,w,CP) (the two seen-mask channels at [E, E + 2)) with the learned deconv
    weight `up_w`: pred (B,H,W) always; loss / stats / confusion counts / d(score) / d(up_w) where given.  ws: a Workspace or None."""
    B, h, w, CP = coarse.shape
    _, H, W = pred.shape
    nbytes = L.load().szn_seenmask_head_workspace_bytes(B, h, w, H, W, CROP)
    buf = _scratch(nbytes, coarse.device) if ws is None else ws.get(nbytes)
    L.call("szn_seenmask_head_k", B, h, w, CP, E, H, W, CROP, L.ptr(coarse), L.ptr(up_w), L.ptr(target), n_class, seen, L.ptr(loss),
           L.ptr(stats), L.ptr(conf), L.ptr(pred), L.ptr(dscore), L.ptr(dup_w), L.ptr(buf),
           L.stream_ptr() if stream is None else stream)


def seenmask_predict(coarse, E, up_w, H, W, target, n_class, seen):
    """forward-only seen-mask head (2-class cross entropy, size_average; seen = seen_set(...)) -> (loss 0-dim tensor, pred (B,H,W)
    int64, 1 = seen)"""
    pred, tgt, loss = _outputs(coarse.shape[0], H, W, coarse.device, target)
    seenmask(coarse, E, up_w, pred, tgt, n_class, seen, loss)
    return loss.reshape(()), pred


def seenmask_group(coarse, E, up_w, H, W):
    """the seen-mask prediction alone (no target, no loss) -> (B,H,W) int64, the group map of cosine() mode 1"""
    gmap = torch.empty(coarse.shape[0], H, W, dtype=torch.int64, device=coarse.device)
    seenmask(coarse, E, up_w, gmap)
    return gmap


def seenmask_margin(coarse, E, up_w, H, W):
    """the seen-mask logit margin s1 - s0 per pixel (szn_seenmask_margin) -> (B,H,W) f32; margin > 0 is seenmask_group's map bit for
    bit, margin > tau the group map of seen_sweep() at threshold tau"""
    B, h, w, CP = coarse.shape
    margin = torch.empty(B, H, W, dtype=torch.float32, device=coarse.device)
    L.call("szn_seenmask_margin", B, h, w, CP, E, H, W, CROP, L.ptr(coarse), L.ptr(up_w), L.ptr(margin), L.stream_ptr())
    return margin
