"""trainer_fcn.py -- phase-1 trainer of the SZN path: FCN backbone + pixel-embedding (or softmax) head.

Same constructor / method surface and return contracts as /root/reference/trainer_fcn.py (Trainer.__init__ :21-81,
forward :83-120, forward_szn :123-147, train_epoch :149-180, validate :182-292, train :294-306), on top of the
HIP path: with an embedding loss 'cos' or the softmax cross entropy (train.py -c 1) the hot loop runs engine.TrainStep
(fused head, flat-buffer optimizer, RCCL gradient all-reduce); other losses compose the same kernels through autograd.  Logging (CSV, optional
tensorboard writer, checkpoints with the reference's dict keys) is host-side and kept format-compatible.
The JPEG tile visualisations of validation (reference :198-219,267; drawn there on the host through the third-party `fcn` package) are
rendered on the GPU by vis_utils from the tensors validate() already holds: Trainer(visualize=N) / train.py --viz N, off by default.
"""
import contextlib
import datetime
import os
import os.path as osp
import shutil

import numpy as np
import torch

from . import engine as _engine
from . import utils
from . import vis_utils
from ._lib import SznError

_DATA = osp.join(osp.dirname(osp.abspath(__file__)), "data")      # package data: .npy re-saves of the reference's pickles


def load_embeddings(dataset, dim):
    """K x E class-embedding matrix: `datasets/<ds>/embeddings/norm_embed_arr_<E>.pkl` relative to the CWD exactly
    like the reference (trainer_fcn.py:49), else the .npy re-saves shipped inside this package (data/)."""
    pkl = 'datasets/%s/embeddings/norm_embed_arr_%s' % (dataset, str(dim))
    if osp.exists(pkl + '.pkl'):
        return np.asarray(utils.load_obj(pkl), dtype=np.float32)
    npy = osp.join(_DATA, "embeddings_%s_%s.npy" % (dataset, str(dim)))
    if osp.exists(npy):
        return np.load(npy)
    raise IOError("no embedding matrix for dataset=%s dim=%s (looked for %s.pkl and %s)" % (dataset, dim, pkl, npy))


_EMBED_LOSSES = ("cos", "mse", "sim_ce", "rank")          # the embedding losses: each has a fused head (heads.embed)


def _now():
    return datetime.datetime.now(datetime.timezone(datetime.timedelta(hours=-5)))      # 'US/Eastern' (no DST handling)


# why a configuration cannot run one of the five inference rules that sweep a scalar: per rule the reasons in the order they are
# tried, each with its whole sentence (the one with %d names the class count).  A rule's sentences are its own: rewording one
# changes that rule alone
_REFUSALS = {
    "calibration": (
        ("unseen", "calibration needs unseen classes (train_unseen / val_unseen): without them there is no seen group to penalise"),
        ("config", "calibration needs an embedding configuration (loss 'cos' | 'mse' | 'sim_ce' | 'rank'): a softmax network has no unseen-class scores"),
        ("forced", "calibration and forced_unseen are two different class-assignment rules: pick one"),
        ("mode", "calibration replaces the seen-mask classifier of -m test_all: use -m test_fcn"),
        ("views", "calibration with eval_scales / eval_flip is not built (the view-ensemble head has no penalty)"),
        ("classes", "calibration: the fused head holds at most 256 classes, got %d"),
        ("verbose", "calibration: SZN_VERBOSE_VAL needs the materialised score, which the calibrated head never forms")),
    "hub": (
        ("unseen", "the hubness correction needs unseen classes (train_unseen / val_unseen): without them there are no two class groups to decide between"),
        ("config", "the hubness correction needs an embedding configuration (loss 'cos' | 'mse' | 'sim_ce' | 'rank'): a softmax network has no unseen-class scores"),
        ("forced", "the hubness correction and forced_unseen are two different class-assignment rules: pick one"),
        ("mode", "the hubness correction replaces the seen-mask classifier of -m test_all: use -m test_fcn"),
        ("views", "the hubness correction with eval_scales / eval_flip is not built (the view-ensemble head has no correction)"),
        ("classes", "the hubness correction: the fused head holds at most 256 classes, got %d"),
        ("verbose", "the hubness correction: SZN_VERBOSE_VAL needs the materialised score, which the corrected head never forms")),
    "seen_threshold": (
        ("unseen", "a seen-mask threshold needs unseen classes (train_unseen / val_unseen): without them there is one class group"),
        ("config", "a seen-mask threshold needs an embedding configuration (loss 'cos' | 'mse' | 'sim_ce' | 'rank'): a softmax network has no class groups"),
        ("forced", "a seen-mask threshold and forced_unseen are two different class-assignment rules: pick one"),
        ("mode", "a seen-mask threshold acts on the full SZN network only: validate(both_fcn_and_seenmask=True), -m test_all"),
        ("views", "a seen-mask threshold with eval_scales / eval_flip is not built (the view-ensemble head takes its own group map)"),
        ("classes", "a seen-mask threshold: the fused head holds at most 256 classes, got %d"),
        ("verbose", "a seen-mask threshold: SZN_VERBOSE_VAL needs the materialised score, which the sweep head never forms")),
    "seen_gate": (
        ("unseen", "the soft seen/unseen gate needs unseen classes (train_unseen / val_unseen): without them there is one class group"),
        ("config", "the soft seen/unseen gate needs an embedding configuration (loss 'cos' | 'mse' | 'sim_ce' | 'rank'): a softmax network has no class groups"),
        ("forced", "the soft seen/unseen gate and forced_unseen are two different class-assignment rules: pick one"),
        ("mode", "the soft seen/unseen gate acts on the full SZN network only: validate(both_fcn_and_seenmask=True), -m test_all"),
        ("views", "the soft seen/unseen gate with eval_scales / eval_flip is not built (the view-ensemble head takes its own group map)"),
        ("classes", "the soft seen/unseen gate: the fused head holds at most 256 classes, got %d"),
        ("verbose", "the soft seen/unseen gate: SZN_VERBOSE_VAL needs the materialised score, which the sweep head never forms")),
    "conse": (
        ("unseen", "conse needs unseen classes (train_unseen / val_unseen): without them the channel argmax already names every class"),
        ("config", "conse needs the softmax configuration (fcn_loss 'cross_entropy', embed_dim 0): an embedding network has heads of its own"),
        ("mode", "conse on the full SZN network (-m test_all, seen-mask grouping) is not built: use -m test_fcn"),
        ("views", "conse with eval_scales / eval_flip is not built (averaging softmax probabilities over views is not)"),
        ("forced", "conse: forced_unseen picks the class group from the target, a gamma or a sweep picks it from the margin: pick one")),
    "ema": (
        ("config", "averaged weights (ema) live in the fused training step's flat buffers: an embedding configuration (loss 'cos' | 'mse' | 'sim_ce' | 'rank') or the softmax configuration (fcn_loss 'cross_entropy', no embedding) only"),
        ("fused", "averaged weights (ema) live in the fused training step's flat buffers (fused_step=True)"),
        ("wiring", "averaged weights (ema) live in the fused training step, which this optimizer wiring does not allow")),
    "clip": (
        ("config", "gradient-norm clipping and the gradient log live in the fused training step: an embedding configuration (loss 'cos' | 'mse' | 'sim_ce' | 'rank') or the softmax configuration (fcn_loss 'cross_entropy', no embedding) only"),
        ("fused", "gradient-norm clipping and the gradient log live in the fused training step (fused_step=True)"),
        ("wiring", "gradient-norm clipping and the gradient log live in the fused training step, which this optimizer wiring does not allow")),
    "accum": (
        ("config", "gradient accumulation sums the fused training step's flat gradient buffers: an embedding configuration (loss 'cos' | 'mse' | 'sim_ce' | 'rank') or the softmax configuration (fcn_loss 'cross_entropy', no embedding) only"),
        ("fused", "gradient accumulation sums the fused training step's flat gradient buffers (fused_step=True)"),
        ("wiring", "gradient accumulation sums the fused training step's gradients, and this optimizer wiring does not run on that step")),
}


def _refused(rule, n_class=0, **holds):
    """the sentence of the first reason of `rule` (_REFUSALS) that holds, or None"""
    for reason, sentence in _REFUSALS[rule]:
        if holds[reason]:
            return sentence % n_class if reason == "classes" else sentence
    return None


def calibration_refused(has_unseen, embed_cfg, forced_unseen, test_all, eval_views, n_class, verbose_val=False):
    """why a configuration cannot run calibrated stacking (calibration= / calib_sweep=, train.py --calibration / --calib-sweep), or
    None: it penalises the seen classes of the plain embedding head, so it needs unseen classes and an embedding configuration, and it
    replaces the other class-assignment rules rather than combining with them"""
    return _refused("calibration", n_class, unseen=not has_unseen, config=not embed_cfg, forced=forced_unseen, mode=test_all,
                    views=eval_views, classes=n_class > 256, verbose=verbose_val)


def seen_threshold_refused(has_unseen, embed_cfg, forced_unseen, test_all, eval_views, n_class, verbose_val=False):
    """why a configuration cannot threshold the seen-mask decision (seen_threshold= / seen_sweep=, train.py --seen-threshold /
    --seen-sweep), or None: the threshold moves the operating point of the full SZN network (validate(True), -m test_all), whose
    seen-mask classifier picks the class group per pixel inside the fused embedding head"""
    return _refused("seen_threshold", n_class, unseen=not has_unseen, config=not embed_cfg, forced=forced_unseen, mode=not test_all,
                    views=eval_views, classes=n_class > 256, verbose=verbose_val)


def seen_gate_refused(has_unseen, embed_cfg, forced_unseen, test_all, eval_views, n_class, verbose_val=False):
    """why a configuration cannot run the soft seen/unseen gate (seen_gate=, train.py --seen-gate), or None: the gate replaces the cut on
    the seen-mask margin by a per-pixel one inside the same sweep head, so seen_threshold_refused's reasons are its reasons"""
    return _refused("seen_gate", n_class, unseen=not has_unseen, config=not embed_cfg, forced=forced_unseen, mode=not test_all,
                    views=eval_views, classes=n_class > 256, verbose=verbose_val)


def hub_refused(has_unseen, embed_cfg, forced_unseen, test_all, eval_views, n_class, verbose_val=False):
    """why a configuration cannot run the hubness correction (hub=, train.py --hub-correct), or None: the correction acts on the
    similarities that enter calibrated stacking's rule inside the same head, so calibration_refused's reasons are its reasons"""
    return _refused("hub", n_class, unseen=not has_unseen, config=not embed_cfg, forced=forced_unseen, mode=test_all,
                    views=eval_views, classes=n_class > 256, verbose=verbose_val)


def conse_refused(has_unseen, softmax_cfg, forced_unseen, test_all, eval_views, tuned):
    """why a configuration cannot run ConSE zero-shot inference (conse= / conse_sweep=, train.py --conse / --conse-sweep), or None: ConSE
    mixes class embeddings with the softmax network's seen-class probabilities, so it needs unseen classes and the softmax
    configuration (cross entropy, no embedding); `tuned` = a gamma other than 0 or a sweep was asked for"""
    return _refused("conse", unseen=not has_unseen, config=not softmax_cfg, mode=test_all, views=eval_views,
                    forced=forced_unseen and tuned)


def ema_refused(step_cfg, fused_step=True, wired=True):
    """why a configuration cannot average its weights (ema=, train.py --ema), or None: the average is kept by engine.TrainStep next to
    its flat parameter buffers, so it exists only where training runs on that step -- step_cfg: loss 'cos' | 'mse' | 'sim_ce' | 'rank'
    with embeddings, or the softmax cross entropy"""
    return _refused("ema", config=not step_cfg, fused=not fused_step, wiring=not wired)


def clip_refused(step_cfg, fused_step=True, wired=True):
    """why a configuration cannot clip by the gradient norm or log gradient statistics (clip_grad_norm= / grad_stats=, train.py
    --clip-grad-norm / --grad-stats), or None: the statistics are taken by engine.TrainStep over its flat gradient buffers, so they
    exist only where training runs on that step (ema_refused's step_cfg); the autograd routes and the seen-mask phase have none"""
    return _refused("clip", config=not step_cfg, fused=not fused_step, wiring=not wired)


def accum_refused(step_cfg, fused_step=True, wired=True):
    """why a configuration cannot accumulate gradients over several iterations (accum_steps=, train.py --accum-steps), or None: the sum
    is kept by engine.TrainStep next to its flat gradient buffers, so it exists only where training runs on that step (ema_refused's
    step_cfg); the autograd routes and the seen-mask phase step after every backward pass"""
    return _refused("accum", config=not step_cfg, fused=not fused_step, wiring=not wired)


def pseudo_refused(has_unseen, embed_cfg, n_class):
    """why a configuration cannot self-train on pseudo labels (pseudo=, train.py --pseudo-label), or None: the labels are the unseen
    classes' calibrated predictions of the fused embedding head"""
    if not has_unseen:
        return "pseudo labels need unseen classes (train_unseen / val_unseen): there is nothing hidden to label"
    if not embed_cfg:
        return "pseudo labels need an embedding configuration (loss 'cos' | 'mse' | 'sim_ce' | 'rank'): a softmax network has no unseen-class scores"
    if n_class > 256:
        return "pseudo labels: the fused head holds at most 256 classes, got %d" % n_class
    return None


def bias_refused(has_unseen, pixel_embeddings, loss_func, n_class):
    """why a configuration cannot train with the unseen-bias loss (bias_loss=, train.py --bias-loss), or None: the term is part of the
    fused sim_ce head and pulls the hidden pixels towards the unseen classes"""
    if not (pixel_embeddings and loss_func == "sim_ce"):
        return "the bias loss belongs to loss 'sim_ce' (got loss %r): it is a term of that head's softmax" % (loss_func,)
    if not has_unseen:
        return "the bias loss needs unseen classes (train_unseen / val_unseen): there is nothing hidden to pull towards them"
    if n_class > 256:
        return "the bias loss: the fused head holds at most 256 classes, got %d" % n_class
    return None


def ohem_refused(embed_cfg, n_class):
    """why a configuration cannot mine hard pixels (ohem=, train.py --ohem), or None: hardness is the cosine to the pixel's own class
    embedding, a quantity of the fused embedding head"""
    if not embed_cfg:
        return "ohem needs an embedding configuration (loss 'cos' | 'mse' | 'sim_ce' | 'rank'): a softmax network has no class embeddings"
    if n_class > 256:
        return "ohem: the fused head holds at most 256 classes, got %d" % n_class
    return None


PROTO_ALPHA = 0.5          # the default of train.py --proto-alpha: the midpoint between word vector and prototype, nobody has tuned it


def proto_refused(has_unseen, embed_cfg, n_class, shots=1):
    """why a configuration cannot adapt its unseen class embeddings from a few labelled shots (proto=, train.py --proto-shots), or None:
    the prototypes are pooled by the fused head's masked-pooling call and replace rows of the class-embedding matrix in validation"""
    if not embed_cfg:
        return "prototype adaptation needs an embedding configuration (loss 'cos' | 'mse' | 'sim_ce' | 'rank'): a softmax network has no class embeddings"
    if not has_unseen:
        return "prototype adaptation needs unseen classes (train_unseen / val_unseen): the seen classes' embeddings are trained against already"
    try:
        ok = int(shots) == shots and int(shots) >= 1
    except (TypeError, ValueError):
        ok = False
    if not ok:
        return "prototype adaptation: shots must be an integer >= 1 (got %r)" % (shots,)
    if n_class > 256:
        return "prototype adaptation: the fused head holds at most 256 classes, got %d" % n_class
    return None


def check_proto(proto):
    """proto = dict(shots=, alpha=PROTO_ALPHA, mode="unit", min_pixels=1) checked -> the dict with every key filled in"""
    from .heads import proto_mode
    if not isinstance(proto, dict) or "shots" not in proto or set(proto) - {"shots", "alpha", "mode", "min_pixels"}:
        raise SznError("proto = dict(shots=N[, alpha=, mode=, min_pixels=]), got %r" % (proto,))
    cfg = dict(alpha=PROTO_ALPHA, mode="unit", min_pixels=1)
    cfg.update({k: v for k, v in proto.items() if v is not None})
    try:
        cfg["shots"], cfg["alpha"], cfg["min_pixels"] = int(cfg["shots"]), float(cfg["alpha"]), int(cfg["min_pixels"])
    except (TypeError, ValueError):
        raise SznError("proto: shots and min_pixels must be integers, alpha a number (got %r)" % (proto,))
    if cfg["shots"] < 1 or cfg["shots"] != proto["shots"]:
        raise SznError("proto: shots must be an integer >= 1 (got %r)" % (proto["shots"],))
    if not 0.0 <= cfg["alpha"] <= 1.0:
        raise SznError("proto: alpha must lie in [0, 1] (got %r)" % (cfg["alpha"],))
    if cfg["min_pixels"] < 1:
        raise SznError("proto: min_pixels must be at least 1 (got %r)" % (cfg["min_pixels"],))
    proto_mode(cfg["mode"])
    return cfg


class _Sweep(object):
    """one sweep of validation -- the calibration gammas, ConSE's gammas, the seen-mask taus: the trainer's candidate values (its
    attribute `attr`, None: no sweep) and the value in use (used() -> a float, or None: none), and while a validation runs (begin ..
    finish) the merged ascending values `all` with their (G,K,K) device histogram `hist`.  With a sweep and a value in use the value
    joins the candidates for the head call (one launch gives both); the rows of the candidates are picked out afterwards."""
    all = hist = None

    def __init__(self, trainer, attr, used, label, noun, fname, tag, best, no_room):
        self.t, self.attr, self.used = trainer, attr, used
        self.label, self.noun, self.fname, self.tag = label, noun, fname, tag        # prints; '<fname>' and its column; tensorboard
        self.best, self.no_room = best, no_room          # the trainer's two best-value attributes; the 64-cap sentence

    def candidates(self):
        return getattr(self.t, self.attr)

    def begin(self):
        used = self.used()
        extra = [] if used is None else [np.float32(used)]
        self.all = np.unique(np.concatenate([self.candidates(), np.asarray(extra, dtype=np.float32)]))
        if self.all.size > 64:
            raise SznError(self.no_room)
        self.hist = torch.zeros(self.all.size, self.t.n_class, self.t.n_class, dtype=torch.int64, device=self.t.device)

    def values(self):
        """what the head call sweeps: the value in use alone outside a sweep"""
        return [self.used()] if self.hist is None else self.all

    def index(self):
        """where the value in use stands among values(), None without one"""
        used = self.used()
        if used is None:
            return None
        return 0 if self.hist is None else int(np.searchsorted(self.all, np.float32(used)))

    def finish(self, world):
        """the validation is over: -> its histogram summed over the ranks as a numpy array, or None outside a sweep.  A collective:
        every rank calls it, for every sweep in the same order"""
        hist, self.hist = self.hist, None
        if hist is None:
            return None
        if world > 1:
            import torch.distributed as dist
            dist.all_reduce(hist)
        return hist.cpu().numpy()

    def scan(self, hist_all):
        """-> ([(value, its (K,K) histogram, metrics, seen metrics, unseen metrics, harmonic mean) per candidate], best): hist_all
        follows `all`; best = the (value, harmonic mean) of the largest harmonic mean, or None; ties go to the value nearest 0 (a NaN
        never wins)"""
        rows, best = [], None
        for val, g in zip(self.candidates(), np.searchsorted(self.all, self.candidates())):
            m, ms, mu = utils.calib_rows(hist_all[g], self.t.n_class, self.t.val_unseen)
            hm = utils.harmonic_mean_iu(ms, mu)
            rows.append((float(val), hist_all[g], m, ms, mu, hm))
            if not np.isnan(hm) and (best is None or hm > best[1] or (hm == best[1] and abs(float(val)) < abs(best[0]))):
                best = (float(val), hm)
        return rows, best

    def keep_best(self, best):
        if best is not None:
            setattr(self.t, self.best[0], best[0])
            setattr(self.t, self.best[1], best[1])

    def report(self, hist_all, fname=None, label=None, detail='', tag=None, extra=()):
        """rank 0, once per validation: one <fname> row per candidate and the candidate with the largest harmonic mean.  fname /
        label / tag: another file, print label or tensorboard tag than the sweep's own; detail follows the label in the best-value
        print; extra: (column, value) pairs appended to every row"""
        t, label, tag = self.t, label or self.label, tag or self.tag
        rows, best = self.scan(hist_all)
        path = osp.join(t.log_dir, fname or self.fname)
        if not osp.exists(path):
            with open(path, 'w') as f:
                f.write(','.join(['epoch,iteration,%s,val/pxl_acc,val/mean_iu,val/seen/mean_iu,val/unseen/mean_iu,val/harmonic_mean_iu' % self.noun]
                                 + [k for k, _ in extra]) + '\n')
        with open(path, 'a') as f:
            for val, _, m, ms, mu, hm in rows:
                f.write(','.join(map(str, [t.epoch, t.iteration, val, m[0], m[2], ms[2], mu[2], hm] + [v for _, v in extra])) + '\n')
        self.keep_best(best)
        if best is not None:
            print('%s%s: best %s %g, harmonic mean IU %.3f' % ((label, detail, self.noun) + best))
            t.tb_writer.add_scalar('%s/best_%s' % (tag, self.noun), best[0], t.epoch)
            t.tb_writer.add_scalar('%s/best_harmonic_mean_iu' % tag, best[1], t.epoch)
        else:
            print('%s: no %s has a harmonic mean IU (the validation set holds no seen or no unseen pixels)' % (label, self.noun))


class _NullWriter(object):
    def add_scalar(self, *a, **k): pass
    def add_text(self, *a, **k): pass
    def add_image(self, *a, **k): pass


class Trainer(object):

    def __init__(self, cuda, model, optimizer, train_loader, val_loader, log_dir, dataset, max_epoch, tb_writer,
                 pixel_embeddings=None, loss_func=None, unseen=None, val_unseen=None, label_names=None,
                 forced_unseen=False, embed_arr=None, precision=torch.float32, fused_step=True, rank=0, visualize=0, augment=None,
                 seen_threshold=None, seen_sweep=None, proto=None, support_loader=None, conse=None, conse_sweep=None, seen_gate=None, hub=None,
                 ema=None, ema_checkpoint=None, clip_grad_norm=None, grad_stats=False, accum_steps=None, sim_temperature=None, rank_margin=None, rank_hardest=False, bias_loss=None, bias_start_epoch=0, pseudo=None, pseudo_start_epoch=0, ohem=None, ohem_start_epoch=0, calibration=None,
                 calib_sweep=None, eval_scales=None, eval_flip=False):
        if not cuda:
            raise RuntimeError("this implementation runs on the GPU only (cuda=False has no CPU fallback)")
        self.cuda = cuda
        self.model = model
        self.optim = optimizer
        self.train_loader = train_loader
        self.val_loader = val_loader
        self.log_dir = log_dir
        self.dataset = dataset
        self.max_epoch = max_epoch
        self.tb_writer = tb_writer if tb_writer is not None else _NullWriter()
        self.pixel_embeddings = pixel_embeddings
        self.loss_func = loss_func
        self.unseen = list(unseen or [])            # all unseen classes (train_unseen + val_unseen)
        self.val_unseen = list(val_unseen or [])
        self.label_names = label_names
        self.forced_unseen = forced_unseen
        self.rank = rank
        self.visualize = int(visualize)             # validation images rendered per epoch (the reference: 25); 0 = none
        self.last_viz = None                        # the last epoch's mosaic, (h, w, 3) uint8 numpy
        # datasets.Augment or None: train_epoch sends every (images, labels, sizes) batch of the training loader (datasets.augment_collate)
        # through it -- random scale / crop / flip on the GPU, a fixed network input size; validate() never augments
        self.augment = augment
        # loss_func "sim_ce" (utils.sim_ce_loss, szn_fused_simce_head): the softmax runs over the seen classes -- its `exclude` is
        # self.unseen -- at this temperature (None: heads.SIM_TEMPERATURE); every fused call reads both from the model
        if sim_temperature is not None and loss_func != "sim_ce":
            raise SznError("sim_temperature belongs to loss 'sim_ce' (got loss %r)" % (loss_func,))
        from .heads import SIM_TEMPERATURE
        self.sim_temperature = float(SIM_TEMPERATURE if sim_temperature is None else sim_temperature)
        if loss_func == "sim_ce" and pixel_embeddings:
            model.set_sim_ce(self.unseen, self.sim_temperature)
        # loss_func "rank" (utils.rank_loss, szn_fused_rank_head): the hinges run over the seen classes -- `exclude` is self.unseen --
        # at this margin (None: heads.RANK_MARGIN), summed or (rank_hardest) the hardest negative alone; the model carries all three
        if (rank_margin is not None or rank_hardest) and loss_func != "rank":
            raise SznError("rank_margin / rank_hardest belong to loss 'rank' (got loss %r)" % (loss_func,))
        from .heads import RANK_MARGIN
        self.rank_margin, self.rank_hardest = float(RANK_MARGIN if rank_margin is None else rank_margin), bool(rank_hardest)
        if loss_func == "rank" and pixel_embeddings:
            model.set_rank(self.unseen, self.rank_margin, self.rank_hardest)
        # multi-scale / mirrored validation (models.ms_predict): the scales every validation image is evaluated at (None: once, as
        # stored) and whether each is also evaluated mirrored.  Training steps never see them.
        self.eval_scales = tuple(float(s) for s in eval_scales) if eval_scales else None
        self.eval_flip = bool(eval_flip)
        self._ms_warned = False
        if (self.eval_scales or self.eval_flip) and not (pixel_embeddings and loss_func in _EMBED_LOSSES):
            raise SznError("eval_scales / eval_flip need an embedding configuration (loss 'cos' | 'mse' | 'sim_ce' | 'rank'): averaging softmax "
                           "probabilities over views is not built")
        if self.eval_flip and not self.eval_scales:
            self.eval_scales = (1.0,)
        # calibrated stacking (models.calib_predict): `calibration` = the penalty gamma subtracted from every seen class's similarity
        # in validation; `calib_sweep` = ascending candidate gammas whose metrics validate() writes to calib_log.csv, one extra head
        # launch per batch.  Training steps never see them.
        self.calibration = None if calibration is None else float(np.float32(calibration))
        self.calib_sweep = None
        if calib_sweep is not None:
            from .heads import calib_gammas
            self.calib_sweep = calib_gammas(calib_sweep)
        self.best_gamma = None
        self.best_harmonic_mean_iu = None
        # hubness correction (models.hub_predict): hub = dict(mode='mean' | 'zscore', beta=, min_sd=) -- validation takes every class's mean
        # similarity over the image's pixels (zscore: and divides by its spread) off the similarities before calibrated stacking's rule, at
        # the gamma of `calibration` (0 without it) and over calib_sweep's gammas; the rows go to hub_log.csv with the hubness (skewness of
        # the per-class prediction counts) of each.  Training steps never see it.
        self.hub = None
        if hub is not None:
            from .heads import hub_params
            self.hub = hub_params(hub)
        self.last_hub_skew = None
        # the seen-mask threshold of the full SZN network (models.seen_sweep_predict), validate(True) only: a pixel takes the seen group
        # iff its seen-mask logit margin s1 - s0 exceeds `seen_threshold` (None: the plain route, which is tau = 0); `seen_sweep` =
        # ascending candidate taus whose metrics validate(True) writes to seen_sweep_log.csv from the same head launch
        self.seen_threshold = None if seen_threshold is None else float(np.float32(seen_threshold))
        self.seen_sweep = None
        if seen_sweep is not None:
            from .heads import seen_sweep_taus
            self.seen_sweep = seen_sweep_taus(seen_sweep)
        self.best_seen_tau = None
        self.best_seen_harmonic_mean_iu = None
        # the soft seen/unseen gate (models.seen_gate_predict), validate(True) only: seen_gate = dict(weight=, temperature=) -- the cut
        # acts on margin - weight * (l_S - l_U), the margin corrected per pixel by how sure the two class experts are, instead of on the
        # margin; seen_threshold / seen_sweep keep their meaning (tau is a cut on that value), the sweep's rows go to seen_gate_log.csv
        self.seen_gate = None
        if seen_gate is not None:
            from .heads import gate_params
            self.seen_gate = dict(zip(("weight", "temperature"), gate_params(seen_gate)))
        self._init_sweeps()

        self.epoch = 0
        self.iteration = 0
        self.best_mean_iu = 0
        self.n_class = len(self.train_loader.dataset.class_names)
        self.timestamp_start = _now()
        self.seen = [x for x in range(self.n_class) if x not in self.unseen]
        self.device = next(model.parameters()).device
        self.precision = precision
        self._step = None
        self._fused_step = fused_step
        self.verbose_val = os.environ.get("SZN_VERBOSE_VAL", "0") == "1"   # per-image prints cost a host sync each
        if self.calibration is not None or self.calib_sweep is not None:
            why = calibration_refused(bool(self.unseen), bool(pixel_embeddings) and loss_func in _EMBED_LOSSES, forced_unseen,
                                      False, bool(self.eval_scales), self.n_class, self.verbose_val)
            if why:
                raise SznError(why)
            if self.calibration is not None and not np.isfinite(self.calibration):
                raise SznError("calibration: gamma must be finite (got %r)" % (calibration,))
        if self.hub is not None:
            why = hub_refused(bool(self.unseen), bool(pixel_embeddings) and loss_func in _EMBED_LOSSES, forced_unseen,
                              False, bool(self.eval_scales), self.n_class, self.verbose_val)
            if why:
                raise SznError(why)
        if self.seen_threshold is not None or self.seen_sweep is not None:
            why = seen_threshold_refused(bool(self.unseen), bool(pixel_embeddings) and loss_func in _EMBED_LOSSES, forced_unseen,
                                         True, bool(self.eval_scales), self.n_class, self.verbose_val)
            if why:
                raise SznError(why)
            if self.seen_threshold is not None and not np.isfinite(self.seen_threshold):
                raise SznError("seen_threshold: tau must be finite (got %r)" % (seen_threshold,))
        if self.seen_gate is not None:
            why = seen_gate_refused(bool(self.unseen), bool(pixel_embeddings) and loss_func in _EMBED_LOSSES, forced_unseen,
                                    True, bool(self.eval_scales), self.n_class, self.verbose_val)
            if why:
                raise SznError(why)

        # ConSE zero-shot inference for the softmax configuration (models.conse_predict): conse = dict(top=, dim=, gamma=) -- validation
        # mixes the dataset's `dim`-wide class embeddings of the top `top` seen classes with their softmax probabilities and names the
        # nearest class, with the penalty `gamma` (default 0) on the seen classes; `conse_sweep` = ascending candidate gammas whose
        # metrics validate() writes to conse_log.csv from the same head launch.  Training steps never see them.
        self.conse = None
        self.conse_sweep = None
        self.conse_embeddings = None
        self.best_conse_gamma = None
        self.best_conse_harmonic_mean_iu = None
        if conse_sweep is not None and conse is None:
            raise SznError("conse_sweep belongs to conse= (ConSE inference), which is off")
        if conse is not None:
            from .heads import calib_gammas, conse_top
            cfg = dict(conse)
            if set(cfg) - {"top", "dim", "gamma"} or "top" not in cfg:
                raise SznError("conse = dict(top=, dim=300, gamma=0.0), got %r" % (conse,))
            gamma = float(np.float32(cfg.get("gamma") or 0.0))
            if not np.isfinite(gamma):
                raise SznError("conse: gamma must be finite (got %r)" % (cfg.get("gamma"),))
            if conse_sweep is not None:
                self.conse_sweep = calib_gammas(conse_sweep)
            why = conse_refused(bool(self.unseen), not pixel_embeddings and loss_func == "cross_entropy", forced_unseen, False,
                                bool(self.eval_scales), gamma != 0.0 or self.conse_sweep is not None)
            if why:
                raise SznError(why)
            if self.conse_sweep is not None and (self.verbose_val or self.n_class > 256):
                raise SznError("conse: a sweep runs on the fused head (at most 256 classes, no SZN_VERBOSE_VAL)")
            if model.n_class != self.n_class:
                raise SznError("conse: the network has %d class channels, the dataset %d classes" % (model.n_class, self.n_class))
            self.conse = dict(top=conse_top(cfg["top"]), dim=int(cfg.get("dim") or 300), gamma=gamma)
            arr = np.asarray(embed_arr, dtype=np.float32) if embed_arr is not None else load_embeddings(dataset, self.conse["dim"])
            if arr.ndim != 2 or arr.shape[0] != self.n_class:
                raise SznError("conse: the class embeddings must be (%d, E), got %r" % (self.n_class, arr.shape))
            self.conse_embeddings = torch.from_numpy(np.ascontiguousarray(arr)).to(self.device).float()

        # self-training (engine.TrainStep pseudo=): from epoch pseudo_start_epoch on every training step labels the most confident
        # `keep` of the hidden pixels (datasets.HIDDEN_LABEL: a hide_unseen training set) per unseen class with the step's own
        # calibrated prediction and trains on them.  pseudo = dict(keep=, gamma=, conf_floor=); the unseen classes are self.unseen,
        # gamma defaults to `calibration`.  Per epoch one row per unseen class in pseudo_log.csv: candidates and selected pixels
        self.pseudo = None
        self.pseudo_start_epoch = int(pseudo_start_epoch)
        if pseudo is not None:
            why = pseudo_refused(bool(self.unseen), bool(pixel_embeddings) and loss_func in _EMBED_LOSSES, self.n_class)
            if why:
                raise SznError(why)
            if not fused_step:
                raise SznError("pseudo labels run inside the fused training step (fused_step=True)")
            cfg = dict(pseudo)
            if cfg.get("gamma") is None:
                cfg["gamma"] = self.calibration if self.calibration is not None else 0.0
            cfg["unseen"] = list(self.unseen)
            _engine.TrainStep._check_pseudo(cfg, loss_func)
            self.pseudo = cfg
            if self.rank == 0:
                os.makedirs(self.log_dir, exist_ok=True)
                if not osp.exists(osp.join(self.log_dir, 'pseudo_log.csv')):
                    with open(osp.join(self.log_dir, 'pseudo_log.csv'), 'w') as f:
                        f.write('epoch,class,candidates,selected\n')

        # hard-pixel mining (engine.TrainStep ohem=): from epoch ohem_start_epoch on every training step trains on the hardest `keep` of
        # each image's labelled pixels (lowest cosine to their own class embedding) and on every pixel below `thresh`.
        # ohem = dict(keep=, thresh=None).  Validation is never mined.  Per epoch one row in ohem_log.csv: evaluated and kept pixels
        self.ohem = None
        self.ohem_start_epoch = int(ohem_start_epoch)
        if ohem is not None:
            why = ohem_refused(bool(pixel_embeddings) and loss_func in _EMBED_LOSSES, self.n_class)
            if why:
                raise SznError(why)
            if not fused_step:
                raise SznError("ohem runs inside the fused training step (fused_step=True)")
            _engine.TrainStep._check_ohem(ohem, loss_func)
            self.ohem = dict(ohem)
            if self.rank == 0:
                os.makedirs(self.log_dir, exist_ok=True)
                if not osp.exists(osp.join(self.log_dir, 'ohem_log.csv')):
                    with open(osp.join(self.log_dir, 'ohem_log.csv'), 'w') as f:
                        f.write('epoch,evaluated,kept,fraction\n')

        # the unseen-bias loss (engine.TrainStep bias=, QFSL): from epoch bias_start_epoch on every hidden pixel (datasets.HIDDEN_LABEL: a
        # hide_unseen training set) adds bias_loss * -log P(unseen classes) to the sim_ce loss; the unseen set is self.unseen.
        # Validation data has no hidden pixels: validation is untouched
        self.bias_loss = None
        self.bias_start_epoch = int(bias_start_epoch)
        if bias_loss is not None:
            from .heads import bias_args
            why = bias_refused(bool(self.unseen), bool(pixel_embeddings), loss_func, self.n_class)
            if why:
                raise SznError(why)
            if not fused_step:
                raise SznError("the bias loss runs inside the fused training step (fused_step=True)")
            cfg = dict(unseen=list(self.unseen), weight=bias_loss)
            bias_args(loss_func, cfg, self.n_class)
            self.bias_loss = cfg

        # averaged weights (engine.TrainStep ema=): ema = dict(decay=, every=1, warmup=True).  Every training step moves an fp32 copy of the
        # parameters towards them on the device; validate() runs entirely on that copy (averaged_weights: val_log.csv, best_mean_iu, every
        # sweep log, the prototypes and the pictures describe the averaged model) and the checkpoint carries it as 'ema_state_dict' /
        # 'ema_updates' next to the raw iterate.  ema_checkpoint: the checkpoint dict a run resumes from -- its average, if it has one,
        # is restored; without one the average starts from the loaded weights.  Per validation one row in ema_log.csv
        self.ema = None
        self._ema_resume = ema_checkpoint if ema is not None else None
        if ema is not None:
            why = ema_refused((bool(pixel_embeddings) and loss_func in _EMBED_LOSSES) or (not pixel_embeddings and loss_func == "cross_entropy"),
                              fused_step)
            if why:
                raise SznError(why)
            decay, every, warm = _engine.TrainStep._check_ema(ema)
            self.ema = dict(decay=decay, every=every, warmup=warm)
            if self.rank == 0:
                os.makedirs(self.log_dir, exist_ok=True)
                if not osp.exists(osp.join(self.log_dir, 'ema_log.csv')):
                    with open(osp.join(self.log_dir, 'ema_log.csv'), 'w') as f:
                        f.write('epoch,iteration,decay,every,updates,rel_l2_distance\n')

        # gradient-norm clipping and the gradient log (engine.TrainStep clip=): clip_grad_norm = MAX > 0 clips every step's gradient to
        # that global L2 norm (torch.nn.utils.clip_grad_norm_'s rule); grad_stats alone measures (MAX = inf).  Either way the
        # per-iteration D2H copy also carries the step's statistics: rank 0 appends one row per iteration to grad_log.csv (its header
        # is written with the first row, from the step's grad_segments) and the progress print shows score_fr's gradient sum
        self.clip = None
        if clip_grad_norm is not None or grad_stats:
            why = clip_refused((bool(pixel_embeddings) and loss_func in _EMBED_LOSSES) or (not pixel_embeddings and loss_func == "cross_entropy"),
                               fused_step)
            if why:
                raise SznError(why)
            self.clip = dict(max_norm=_engine.TrainStep._check_clip(dict(max_norm=float('inf') if clip_grad_norm is None else clip_grad_norm)))

        # gradient accumulation (engine.TrainStep accum=): accum_steps = A >= 1 loader batches per optimizer step.  An iteration stays
        # one loader batch (one micro-step): train_log.csv, the progress print and self.iteration keep their meaning, a grad_log.csv
        # row is written for the iterations that ran the optimizer, and a window is carried across the end of an epoch.  The update
        # uses the mean of the window's gradients, except under the reference's pixel-SUM cross entropy (train.py -c 1), where a larger
        # batch grows the gradient the same way: there it uses their sum.  Validation and checkpoints in the middle of a window are
        # fine (they touch neither the gradient buffers nor the accumulators); a resumed run restarts its window
        self.accum = None
        if accum_steps is not None:
            why = accum_refused((bool(pixel_embeddings) and loss_func in _EMBED_LOSSES) or (not pixel_embeddings and loss_func == "cross_entropy"),
                                fused_step)
            if why:
                raise SznError(why)
            steps, average = _engine.TrainStep._check_accum(dict(steps=accum_steps, average=bool(pixel_embeddings)))
            self.accum = dict(steps=steps, average=average)

        if self.pixel_embeddings:
            arr = np.asarray(embed_arr, dtype=np.float32) if embed_arr is not None else \
                load_embeddings(dataset, pixel_embeddings)
            self.embeddings = torch.from_numpy(arr).to(self.device).float()
            # zero-masked copies used for forced_unseen / full SZN testing (reference :56-64; built in float64)
            seen_arr, unseen_arr = np.zeros(arr.shape), np.zeros(arr.shape)
            seen_arr[self.seen, :] = arr[self.seen, :]
            unseen_arr[self.unseen, :] = arr[self.unseen, :]
            self.seen_embeddings = torch.from_numpy(seen_arr).to(self.device).float()
            self.unseen_embeddings = torch.from_numpy(unseen_arr).to(self.device).float()

        # few-shot prototype adaptation (models.class_prototypes, utils.blend_prototypes): every validate() pools the prototypes of
        # self.unseen over `support_loader` (a loader over datasets.SupportSet: `shots` one-class masks per unseen class) with the current
        # weights and evaluates with those rows of the class embeddings moved `alpha` of the way from the word vector to the prototype.
        # proto = dict(shots=, alpha=, mode=, min_pixels=).  Training steps never see the adapted rows.  Per validation one row per
        # unseen class in proto_log.csv
        self.proto = None
        self.support_loader = support_loader
        self.last_proto = None                       # the last validation's (sums, counts) as numpy arrays
        if proto is not None:
            why = proto_refused(bool(self.unseen), self._embed_cfg(), self.n_class, proto.get("shots", 1) if isinstance(proto, dict) else 1)
            if why:
                raise SznError(why)
            self.proto = check_proto(proto)
            if support_loader is None:
                raise SznError("proto needs support_loader: a loader over datasets.SupportSet(base, unseen classes, shots)")
            if self.rank == 0:
                os.makedirs(self.log_dir, exist_ok=True)
                if not osp.exists(osp.join(self.log_dir, 'proto_log.csv')):
                    with open(osp.join(self.log_dir, 'proto_log.csv'), 'w') as f:
                        f.write('epoch,class,name,shots,participating,contributing,cos_word_proto\n')
        elif support_loader is not None:
            raise SznError("support_loader belongs to proto= (prototype adaptation), which is off")

        base = ['loss', 'pxl_acc', 'class_acc', 'mean_iu', 'fwavacc']
        self.train_log_headers = ['epoch', 'iteration'] + ['train/' + b for b in base] + ['elapsed_time']
        self.val_log_headers = ['epoch', 'iteration'] + ['val/' + b for b in base]
        if self.unseen:
            for grp in ('seen', 'unseen'):
                self.val_log_headers += ['val/%s/%s' % (grp, b) for b in base[1:]]
        self.val_log_headers += ['elapsed_time']
        if self.rank == 0:
            os.makedirs(self.log_dir, exist_ok=True)
            for fname, hdr in (('train_log.csv', self.train_log_headers), ('val_log.csv', self.val_log_headers)):
                if not osp.exists(osp.join(self.log_dir, fname)):
                    with open(osp.join(self.log_dir, fname), 'w') as f:
                        f.write(','.join(hdr) + '\n')

    # ---- forward passes ------------------------------------------------------------------------------------
    def _unpack(self, data, target):
        """targets are (label, label_embedding) tuples when embeddings are on (dataset contract, context_dataset.py:
        116-141); the dense per-pixel embedding is optional here: the label alone is enough (gathered on the GPU)."""
        target_embed = None
        if self.pixel_embeddings and isinstance(target, (tuple, list)):
            target, target_embed = target
        if data.dtype == torch.uint8:              # native dataset samples: raw RGB (n,h,w,3); BGR - mean on the GPU
            data = utils.image_to_device(data, self.device)
        else:
            data = data.to(self.device, non_blocking=True)
        target = target.to(self.device, non_blocking=True)
        if target_embed is not None:
            if target_embed.dim() == 4 and target_embed.is_floating_point():
                target_embed = target_embed.to(self.device, non_blocking=True)     # the reference's dense (n,E,h,w) volume
            else:
                target_embed = None            # label-only datasets: the row of the K x E matrix is gathered on the GPU
        return data, target, target_embed

    def _loss(self, score, target, target_embed):
        te = target_embed if target_embed is not None else (self.embeddings if self.pixel_embeddings else None)
        if self.loss_func == "cos":
            return utils.cosine_loss(score, target, te)
        if self.loss_func == "mse":
            return utils.mse_loss(score, target, te)
        if self.loss_func == "sim_ce":
            return utils.sim_ce_loss(score, target, self.embeddings, self.unseen, self.sim_temperature)
        if self.loss_func == "rank":
            return utils.rank_loss(score, target, self.embeddings, self.unseen, self.rank_margin, self.rank_hardest)
        if self.loss_func == "cross_entropy":
            return utils.cross_entropy2d(score, target, size_average=False)
        raise ValueError("unknown loss_func %r" % (self.loss_func,))

    def forward(self, data, target):
        """-> (score, loss, lbl_pred numpy int64 (n,h,w), lbl_true cpu tensor)   [reference :83-120]"""
        data, target, target_embed = self._unpack(data, target)
        score = self.model(data, mode='fcn')
        loss = self._loss(score, target, target_embed)
        if np.isnan(float(loss.item())):
            raise ValueError('loss is nan while training')
        if self.pixel_embeddings:
            if self.forced_unseen:
                lbl_pred = utils.infer_lbl_forced_unseen(score, target, self.seen_embeddings, self.unseen_embeddings,
                                                         self.unseen, self.cuda)
            else:
                lbl_pred = utils.infer_lbl(score, self.embeddings, self.cuda)
        else:
            lbl_pred = utils.channel_argmax(score).cpu().numpy()
        return score, loss, lbl_pred, target.detach().cpu()

    def forward_szn(self, data, target):
        """both heads + seen-mask-stitched inference   [reference :123-147]"""
        data, target, target_embed = self._unpack(data, target)
        fcn_score, seen_mask_score = self.model(data, mode='both')
        loss = self._loss(fcn_score, target, target_embed)
        lbl_pred = utils.infer_lbl_szn(fcn_score, seen_mask_score, self.seen_embeddings, self.unseen_embeddings, self.cuda)
        return fcn_score, loss, lbl_pred, target.detach().cpu()

    # ---- training --------------------------------------------------------------------------------------------
    def _embed_cfg(self):
        """an embedding configuration whose loss has a fused head: cosine, mse, sim_ce or rank (train.py -loss cos | mse | sim_ce | rank)"""
        return bool(self.pixel_embeddings) and self.loss_func in _EMBED_LOSSES

    def _ce_cfg(self):
        """the softmax configuration (train.py -c 1): cross entropy over the model's own n_class channels, at most 256 classes"""
        return (not self.pixel_embeddings and self.loss_func == "cross_entropy" and self.n_class <= 256
                and self.model.n_class == self.n_class)

    def _fast_step(self):
        """engine.TrainStep when the configuration allows it: embedding cosine or mse loss (forced_unseen: the step's prediction is the
        forced-unseen one, trainer_fcn.py:110-112) or the softmax cross entropy (_ce_cfg), and an optimizer with exactly the reference's two parameter groups
        (train.py:126-133: all Conv2d weights | all Conv2d biases).  Hyper-parameters are read per group from the optimizer object; any other wiring keeps the autograd path."""
        if self._step is not None or not (self._fused_step and (self._embed_cfg() or self._ce_cfg())):
            return self._step
        from .optim import FusedAdam, FusedSGD
        from .models import opt_layers
        _OPT_LAYERS = opt_layers(self.model)
        groups = self.optim.param_groups
        ws = [getattr(self.model, n).weight for n in _OPT_LAYERS]
        bs = [getattr(self.model, n).bias for n in _OPT_LAYERS]
        same = lambda a, b: len(a) == len(b) and {id(t) for t in a} == {id(t) for t in b}
        if len(groups) != 2 or not same(groups[0]['params'], ws) or not same(groups[1]['params'], bs):
            return None
        gw, gb = groups
        if isinstance(self.optim, (FusedAdam, torch.optim.Adam)):
            if gw.get('amsgrad') or gw['betas'] != gb['betas'] or gw['eps'] != gb['eps']:
                return None
            kw = dict(optimizer="adam", betas=tuple(gw['betas']), eps=gw['eps'], adam_weight_decay=gw.get('weight_decay', 0.0))
        elif isinstance(self.optim, (FusedSGD, torch.optim.SGD)):
            if gw.get('nesterov') or gw.get('dampening', 0) or gw.get('momentum', 0) != gb.get('momentum', 0):
                return None
            kw = dict(optimizer="sgd", momentum=gw.get('momentum', 0), weight_decay=gw.get('weight_decay', 0.0))
        else:
            return None
        if self._ce_cfg():
            # the softmax FCN (train.py -c 1): fused cross-entropy head, summed loss (self._loss), channel-argmax prediction
            kw.update(loss="cross_entropy", size_average=False)
        else:
            kw.update(embeddings=self.embeddings, forced_unseen=self.unseen if self.forced_unseen else None, loss=self.loss_func)
            if self.loss_func == "sim_ce":
                kw.update(sim_exclude=self.unseen, sim_temperature=self.sim_temperature)
            if self.loss_func == "rank":
                kw.update(sim_exclude=self.unseen, rank_margin=self.rank_margin, rank_hardest=self.rank_hardest)
            if self.pseudo is not None:
                kw.update(pseudo=self.pseudo)
            if self.ohem is not None:
                kw.update(ohem=self.ohem)
            if self.bias_loss is not None:
                kw.update(bias=self.bias_loss)
        if self.ema is not None:
            kw.update(ema=self.ema)
        if self.clip is not None:
            kw.update(clip=self.clip)
        if self.accum is not None:
            kw.update(accum=self.accum)
        self._step = _engine.TrainStep(self.model, lr=gw['lr'], bias_lr=gb['lr'],
                                       bias_weight_decay=gb.get('weight_decay', 0.0), precision=self.precision,
                                       fused_head=True, keep_grads=os.environ.get("SZN_KEEP_GRADS", "0") == "1", **kw)
        # keep_grads=False (default; SZN_KEEP_GRADS=1 restores the reference's "`.grad` valid until zero_grad()"): the loop
        # calls zero_grad() next (train.py:170-175) and nothing reads the weight gradients in between, so the layers whose Adam
        # step rides in their weight-gradient kernel do not store theirs -- those `.grad`s are None, not stale
        self._step.import_optimizer_state(self.optim)       # resumed runs (train.py:135-136)
        if self.ema is not None and self._ema_resume is not None and 'ema_state_dict' in self._ema_resume:
            # the checkpoint carries an average: restore it (without one import_optimizer_state started it from the loaded weights)
            self._step.load_ema_state_dict(self._ema_resume['ema_state_dict'])
            self._step.ema_updates = int(self._ema_resume.get('ema_updates', 0))
        self._ema_resume = None
        return self._step

    def _ema_step(self):
        """the fused step that keeps the average (ema=), built if need be; an SznError where this optimizer wiring has none"""
        step = self._fast_step()
        if step is None:
            raise SznError(ema_refused(True, True, False))
        return step

    def train_epoch(self):
        self.model.train()
        step = self._fast_step()
        if self.ema is not None:
            self._ema_step()
        if self.clip is not None and step is None:
            raise SznError(clip_refused(True, True, False))
        if self.accum is not None and step is None:
            raise SznError(accum_refused(True, True, False))
        if self.pseudo is not None:
            if step is None:
                raise SznError("pseudo labels run inside the fused training step, which this optimizer wiring does not allow")
            step.set_pseudo_active(self.epoch >= self.pseudo_start_epoch)
            step.pseudo_counts.zero_()
        if self.ohem is not None:
            if step is None:
                raise SznError("ohem runs inside the fused training step, which this optimizer wiring does not allow")
            step.set_ohem_active(self.epoch >= self.ohem_start_epoch)
            step.ohem_counts.zero_()
        if self.bias_loss is not None:
            if step is None:
                raise SznError("the bias loss runs inside the fused training step, which this optimizer wiring does not allow")
            step.set_bias_active(self.epoch >= self.bias_start_epoch)
        if step is None and self.model._engine.dtype == torch.float16:
            # IEEE-half gradients need loss scaling, which only engine.TrainStep applies (d(coarse) is multiplied in fp32 before
            # it enters the 16-bit backward pass); the autograd paths (non-reference optimizer wiring, more than 256 classes)
            # would push ~1e-7-sized activation gradients through fp16 unscaled and lose them silently
            raise RuntimeError("precision fp16 is only supported on the fused training step (embedding cosine / mse loss or "
                               "softmax cross entropy, reference optimizer wiring); use bf16 or fp32 for this configuration")
        for batch_idx, batch in enumerate(self.train_loader):
            if self.augment is not None:
                data, target = self.augment.apply(batch, self.epoch, self.iteration, self.rank, self.device)
            else:
                data, target = batch[:2]             # (an augment_collate loader without augment= is the padded route: sizes unused)
            if step is not None:
                data, target, _ = self._unpack(data, target)
                step.hist.zero_()
                loss, pred = step.step(data, target)
                # one D2H per iteration: the loss and the K x K histogram the step already accumulated on the device
                # (the reference logs per-iteration metrics, trainer_fcn.py:164-174)
                parts = [loss.reshape(1).double(), step.hist[0].reshape(-1).double()]
                if self.clip is not None:            # the step's gradient statistics ride in the same copy
                    parts += [step.grad_stats.reshape(-1), step.clip_state.double(), step.clip_scale.double()]
                packed = torch.cat(parts).cpu().numpy()
                lossv = float(packed[0])
                gsum = float('nan')                  # not read back on this path (a host sync per iteration for a debug print)
                if self.clip is not None and step.last_applied:      # (before the NaN check: the row of the step that broke is the one to
                    # look at; under accum_steps the iterations that only summed their gradient took no statistics and write no row)
                    gsum = self._grad_log(step, packed[1 + self.n_class * self.n_class:])
                if np.isnan(lossv):
                    raise ValueError('loss is nan while training')
                metrics = utils._hist_to_metrics(packed[1:1 + self.n_class * self.n_class].reshape(self.n_class, self.n_class))
                ssum = float('nan')                  # the (B,E,H,W) score is never materialised on this path
            elif (hasattr(self.model, 'embed_loss') and self._fused_step and self._embed_cfg()
                  and not self.forced_unseen and self.embeddings.shape[0] <= 256):
                # FCN8s: autograd chain with the fused-from-1/8-map head (no (n,E,h,w) score), per-tensor fused optimizer
                data, target, _ = self._unpack(data, target)
                loss, pred = self.model.embed_loss(data, self.embeddings, target, loss=self.loss_func)
                self.optim.zero_grad()
                loss.backward()
                _engine.allreduce_param_grads([p for g in self.optim.param_groups for p in g['params']])
                self.optim.step()
                hist = utils.confusion_hist_device(target, pred, self.n_class)[0]
                packed = torch.cat([loss.detach().reshape(1).double(), hist.reshape(-1).double()]).cpu().numpy()
                lossv = float(packed[0])
                if np.isnan(lossv):
                    raise ValueError('loss is nan while training')
                metrics = utils._hist_to_metrics(packed[1:].reshape(self.n_class, self.n_class))
                gsum = ssum = float('nan')
            else:
                score, loss, lbl_pred, lbl_true = self.forward(data, target)
                self.optim.zero_grad()
                loss.backward()
                # data parallel: mean of the rank gradients before the update (the fused path does this inside TrainStep)
                _engine.allreduce_param_grads([p for g in self.optim.param_groups for p in g['params']])
                self.optim.step()
                lossv = float(loss.item())
                metrics = utils.label_accuracy_score(lbl_true.numpy(), lbl_pred, self.n_class)
                gsum = float(self.model.score_fr.weight.grad.sum().item())
                ssum = float(score.sum().item())
            if self.rank == 0:
                print("FCN Train Epoch {:<5} | Iteration {:<5} | Loss {:5.5f} | score_fr grad sum {:15.0f} | "
                      "upscore grad sum {:15.0f} | score sum {:10.5f}".format(int(self.epoch), int(batch_idx), lossv, gsum,
                                                                               0.0, ssum))
                with open(osp.join(self.log_dir, 'train_log.csv'), 'a') as f:
                    elapsed = (_now() - self.timestamp_start).total_seconds()
                    f.write(','.join(map(str, [self.epoch, self.iteration, lossv] + list(metrics) + [elapsed])) + '\n')
                for name, v in zip(['loss', 'pxl_acc', 'class_acc', 'mean_iu', 'fwavacc'], [lossv] + list(metrics)):
                    self.tb_writer.add_scalar('fcn/train/' + name, v, self.iteration)
            self.iteration += 1
        if self.pseudo is not None:
            self._pseudo_report(step)
        if self.ohem is not None:
            self._ohem_report(step)

    def _grad_log(self, step, tail):
        """one grad_log.csv row (rank 0) from the tail of the iteration's D2H copy: grad_stats, clip_state, the loss scale the
        gradients carried -> score_fr's gradient sum for the progress print (trainer_fcn.py:160-162 of the reference)"""
        names = step.grad_segments
        ns = len(names)
        r = _engine.grad_report(names, tail[:2 * ns].reshape(ns, 2), tail[2 * ns:2 * ns + 4], step.grad_factor() / float(tail[2 * ns + 4]))
        if self.rank == 0:
            path = osp.join(self.log_dir, 'grad_log.csv')
            new = not osp.exists(path)
            with open(path, 'a') as f:
                if new:
                    f.write(','.join(['epoch', 'iteration', 'grad_norm', 'clip_coef', 'clipped_steps'] + names) + '\n')
                f.write(','.join(map(str, [self.epoch, self.iteration, r["norm"], r["coef"], r["clipped"]]
                                     + [r["norms"][n] for n in names])) + '\n')
        return r["sums"]["score_fr.weight"]

    def _ohem_report(self, step):
        """once per epoch: the step's {evaluated, kept} pixel counts, summed over the ranks, as one ohem_log.csv row (rank 0)"""
        import torch.distributed as dist
        counts = step.ohem_counts.clone()
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(counts)
        n, kept = (int(v) for v in counts.cpu().numpy())
        self.last_ohem_counts = (n, kept)
        if self.rank == 0:
            with open(osp.join(self.log_dir, 'ohem_log.csv'), 'a') as f:
                f.write('%d,%d,%d,%.6f\n' % (self.epoch, n, kept, kept / n if n else 1.0))

    def _pseudo_report(self, step):
        """once per epoch: the step's {candidates, selected} counts per class, summed over the ranks, as pseudo_log.csv rows (rank 0)"""
        import torch.distributed as dist
        counts = step.pseudo_counts.clone()
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(counts)
        counts = counts.cpu().numpy()
        self.last_pseudo_counts = counts
        if self.rank == 0:
            with open(osp.join(self.log_dir, 'pseudo_log.csv'), 'a') as f:
                for k in self.unseen:
                    f.write('%d,%d,%d,%d\n' % (self.epoch, k, counts[k, 0], counts[k, 1]))

    def _predict_device(self, data, target, szn, with_image=False):
        """forward + loss + class assignment with everything left on the GPU -> (score, loss 0-dim, pred (n,h,w), target), and with
        `with_image` the device image the network read (n,3,h,w) as a fifth element (what validate() renders)"""
        data, target, target_embed = self._unpack(data, target)
        out = self._predict_unpacked(data, target, target_embed, szn)
        return out + (data,) if with_image else out

    def _predict_unpacked(self, data, target, target_embed, szn):
        if (self._embed_cfg() and not szn and not self.forced_unseen and target_embed is None
                and not self.verbose_val and self.embeddings.shape[0] <= 256):
            # plain embedding inference: loss + class assignment straight from the 1/32 map (no (n,E,h,w) score in HBM)
            if self.eval_scales:
                loss, pred = self.model.ms_predict(data, self.embeddings, self.eval_scales, self.eval_flip, target, loss=self.loss_func)
                return None, loss, pred, target
            if self.hub is not None:
                # hubness correction: calibrated stacking's route with szn_hub_stats + szn_hub_head; without a calibration gamma = 0
                loss, pred, _ = self.model.hub_predict(data, self.embeddings, self.unseen, self.hub, self._calib.values(), target,
                                                       hist=self._calib.hist, pred_index=self._calib.index(), loss=self.loss_func)
                return None, loss, pred, target
            if self.calibration is not None or self._calib.hist is not None:
                # calibrated stacking: the penalised classes are those not in self.unseen.  One forward pass; the sweep's histogram
                # and the calibrated prediction come from szn_calib_head launches on the map the loss used
                loss, pred, _ = self.model.calib_predict(data, self.embeddings, self.unseen, self._calib.values(), target,
                                                         hist=self._calib.hist, pred_index=self._calib.index(), loss=self.loss_func)
                return None, loss, pred, target
            loss, pred = self.model.embed_predict(data, self.embeddings, target, loss=self.loss_func)
            return None, loss, pred, target
        if (self._embed_cfg() and (szn or self.forced_unseen) and target_embed is None
                and not self.verbose_val and self.embeddings.shape[0] <= 256):
            # full SZN network (seen-mask-stitched) or forced-unseen inference, same route: the seen-mask group (or the target's)
            # picks the class subset per pixel inside the fused head -- neither (n,E,h,w) nor (n,2,h,w) score in HBM
            if self.eval_scales:
                loss, pred = self.model.ms_predict(data, self.embeddings, self.eval_scales, self.eval_flip, target, unseen=self.unseen,
                                                   group='seenmask' if szn else 'target', loss=self.loss_func)
                return None, loss, pred, target
            if szn and self.seen_gate is not None:
                # the soft gate: the same route with szn_soft_gate_head; without a threshold the reported prediction is tau = 0's
                loss, pred, _ = self.model.seen_gate_predict(data, self.embeddings, self.unseen, self._seen.values(), self.seen_gate, target,
                                                             hist=self._seen.hist, pred_index=self._seen.index(), loss=self.loss_func)
                return None, loss, pred, target
            if szn and (self.seen_threshold is not None or self._seen.hist is not None):
                # the seen-mask decision at a threshold: one forward pass; the sweep's histogram and the reported prediction come from
                # one szn_seen_sweep_head launch on the map the loss used
                loss, pred, _ = self.model.seen_sweep_predict(data, self.embeddings, self.unseen, self._seen.values(), target,
                                                              hist=self._seen.hist, pred_index=self._seen.index(), loss=self.loss_func)
                return None, loss, pred, target
            predict = {"cos": self.model.szn_predict, "mse": self.model.szn_predict_mse,
                       "sim_ce": self.model.szn_predict_sim_ce, "rank": self.model.szn_predict_rank}[self.loss_func]
            loss, pred = predict(data, self.embeddings, self.unseen, target, group='seenmask' if szn else 'target')
            return None, loss, pred, target
        if szn and (self.seen_threshold is not None or self._seen.hist is not None or self.seen_gate is not None):
            raise SznError("a seen-mask threshold runs on the fused head: dense target embeddings keep the materialised score")
        if self.eval_scales and not self._ms_warned:
            # dense target embeddings, SZN_VERBOSE_VAL and more than 256 classes keep the materialised-score route: one view
            self._ms_warned = True
            print("warning: eval_scales / eval_flip ignored: this validation route materialises the score and evaluates one view")
        if self.conse is not None and szn:
            raise SznError(conse_refused(True, True, False, True, False, False))
        if self._ce_cfg() and self._fused_step and not szn and not self.verbose_val:
            if self.conse is not None:
                # ConSE: the loss is softmax_predict's; the class comes from szn_conse_head on the same map (no score, softmax,
                # mixture or cosine in HBM), forced by the target under forced_unseen, else at the gamma in use with the sweep's histogram
                if self.forced_unseen:
                    loss, pred, _ = self.model.conse_predict(data, self.conse_embeddings, self.unseen, self.conse["top"], target=target,
                                                             forced=True)
                else:
                    loss, pred, _ = self.model.conse_predict(data, self.conse_embeddings, self.unseen, self.conse["top"],
                                                             self._conse.values(), target, hist=self._conse.hist,
                                                             pred_index=self._conse.index())
                return None, loss, pred, target
            # softmax inference: summed cross entropy + channel argmax straight from the coarse map (no (n,C,h,w) score in HBM)
            loss, pred = self.model.softmax_predict(data, target)
            return None, loss, pred, target
        if self.conse is not None and self._conse.hist is not None:
            raise SznError("conse: a sweep runs on the fused head; this validation route materialises the score")
        if szn:
            score, seen_mask_score = self.model(data, mode='both')
        else:
            score = self.model(data, mode='fcn')
        loss = self._loss(score, target, target_embed)
        if self.conse is not None:
            # the materialised route (more than 256 classes, SZN_VERBOSE_VAL, fused_step off): the torch-op referee on the score
            pred = utils.conse_infer(score, self.conse_embeddings, self.unseen, self.conse["top"], self.conse["gamma"],
                                     target if self.forced_unseen else None)
        elif not self.pixel_embeddings:
            pred = utils.channel_argmax(score)
        elif szn:
            full = self.seen_embeddings + self.unseen_embeddings
            pred = utils.infer_lbl_device(score, full, mode=1, unseen=self.unseen, seenmask=seen_mask_score)
        elif self.forced_unseen:
            full = self.seen_embeddings + self.unseen_embeddings
            pred = utils.infer_lbl_device(score, full, mode=1, unseen=self.unseen, target=target)
        else:
            pred = utils.infer_lbl_device(score, self.embeddings)
        return score, loss, pred, target

    def _init_sweeps(self):
        """the three sweeps of validation, in the fixed order every rank begins, finishes (a collective each) and reports them.  The
        hubness correction runs on calib's sweep (gamma 0 in use without a calibration), the soft gate on seen's"""
        self._calib = _Sweep(self, 'calib_sweep', self._calib_used, 'calibration', 'gamma', 'calib_log.csv', 'fcn/val/calib',
                             ('best_gamma', 'best_harmonic_mean_iu'),
                             "calibration: a 64-gamma sweep has no room for a calibration value that is not one of its gammas")
        self._seen = _Sweep(self, 'seen_sweep', lambda: 0.0 if self.seen_threshold is None else self.seen_threshold,
                            'seen-mask threshold', 'tau', 'seen_sweep_log.csv', 'fcn/val/seen_sweep',
                            ('best_seen_tau', 'best_seen_harmonic_mean_iu'),
                            "seen sweep: a 64-tau sweep has no room for a reported threshold (seen_threshold, else 0) that is not one of its taus")
        self._conse = _Sweep(self, 'conse_sweep', lambda: self.conse["gamma"], 'conse', 'gamma', 'conse_log.csv', 'fcn/val/conse',
                             ('best_conse_gamma', 'best_conse_harmonic_mean_iu'),
                             "conse: a 64-gamma sweep has no room for a gamma in use that is not one of its gammas")
        self._sweeps = (self._calib, self._seen, self._conse)

    def _calib_used(self):
        return 0.0 if self.hub is not None and self.calibration is None else self.calibration

    def _hub_report(self, h, hist_all):
        """rank 0, once per validation: hub_log.csv -- one 'used' row for the prediction validation reports (h: the {all, seen, unseen}
        histograms) and one 'sweep' row per gamma of calib_sweep (hist_all, or None), each with the hubness of its prediction"""
        path = osp.join(self.log_dir, 'hub_log.csv')
        if not osp.exists(path):
            with open(path, 'w') as f:
                f.write('epoch,iteration,row,mode,beta,min_sd,gamma,val/mean_iu,val/seen/mean_iu,val/unseen/mean_iu,val/harmonic_mean_iu,'
                        'val/hubness_skew\n')
        head = [self.epoch, self.iteration]
        cfg = [self.hub["mode"], self.hub["beta"], self.hub["min_sd"]]
        rows, best = self._calib.scan(hist_all) if hist_all is not None else ([], None)
        with open(path, 'a') as f:
            m, ms, mu = (utils._hist_to_metrics(x) for x in h)
            self.last_hub_skew = utils.hubness_skew(h[0])
            f.write(','.join(map(str, head + ['used'] + cfg + [self._calib_used(), m[2], ms[2], mu[2], utils.harmonic_mean_iu(ms, mu),
                                                                self.last_hub_skew])) + '\n')
            for val, hist, m, ms, mu, hm in rows:
                f.write(','.join(map(str, head + ['sweep'] + cfg + [val, m[2], ms[2], mu[2], hm, utils.hubness_skew(hist)])) + '\n')
        self.tb_writer.add_scalar('fcn/val/hub/skew', self.last_hub_skew, self.epoch)
        self._calib.keep_best(best)
        if best is not None:
            print('hubness correction (%s): best gamma %g, harmonic mean IU %.3f' % ((self.hub["mode"],) + best))

    def _gate_report(self, hist_all):
        """the seen sweep's report with the soft gate on: the rows go to seen_gate_log.csv, which also names the gate's weight and temperature"""
        g = self.seen_gate
        self._seen.report(hist_all, 'seen_gate_log.csv', 'soft gate', ' (weight %g, temperature %g)' % (g["weight"], g["temperature"]),
                          'fcn/val/seen_gate', (('weight', g["weight"]), ('temperature', g["temperature"])))

    def pool_prototypes(self):
        """the prototypes of self.unseen pooled over the support loader with the current weights: one inference forward per support
        batch, accumulated on the device -> (sums (K,E) float64, counts (K,2) int64, shots (K,) int64: support samples that showed the
        class).  Every rank pools the whole (small) support set itself: nothing is exchanged."""
        self.model.eval()
        out = None
        shots = torch.zeros(self.n_class, dtype=torch.int64, device=self.device)
        cls = torch.tensor(self.unseen, dtype=torch.int64, device=self.device)
        with torch.no_grad():
            for batch in self.support_loader:
                data, target, _ = self._unpack(batch[0], batch[1])
                res = self.model.class_prototypes(data, target, self.n_class, self.unseen, self.proto["mode"], out)
                out = res if out is None else out
                shots[cls] += (target.reshape(target.shape[0], 1, -1) == cls.reshape(1, -1, 1)).any(dim=2).sum(dim=0)
        if out is None:
            E = self.embeddings.shape[1]
            out = (torch.zeros(self.n_class, E, dtype=torch.float64, device=self.device),
                   torch.zeros(self.n_class, 2, dtype=torch.int64, device=self.device))
        return out[0], out[1], shots

    def _proto_report(self, sums, counts, shots):
        """rank 0, once per validation: one proto_log.csv row per unseen class"""
        e = self._proto_saved[0].detach().cpu().numpy().astype(np.float64)
        with open(osp.join(self.log_dir, 'proto_log.csv'), 'a') as f:
            for k in self.unseen:
                with np.errstate(invalid="ignore", divide="ignore"):
                    cosv = float(np.dot(e[k], sums[k]) / (np.linalg.norm(e[k]) * np.linalg.norm(sums[k])))
                name = str(self.label_names[k]) if self.label_names is not None and k < len(self.label_names) else 'class%d' % k
                f.write('%d,%d,%s,%d,%d,%d,%r\n' % (self.epoch, k, name.replace(',', ' '), shots[k], counts[k, 0], counts[k, 1], cosv))

    ema = None                                  # dict(decay, every, warmup) with ema=
    _proto_saved = None                         # (embeddings, seen_embeddings, unseen_embeddings) while the adapted rows are swapped in

    @contextlib.contextmanager
    def adapted_embeddings(self):
        """proto=: for the duration of the block self.embeddings (and its row-zeroed companions seen_embeddings / unseen_embeddings)
        are fresh tensors whose unseen rows are blended with the prototypes pooled just now (pool_prototypes, utils.blend_prototypes);
        the originals return in a `finally`.  Fresh tensors: heads.Workspace.prepared sees new keys.  Without proto= nothing happens."""
        if self.proto is None or self._proto_saved is not None:
            yield
            return
        sums, counts, shots = self.pool_prototypes()
        adapted = utils.blend_prototypes(self.embeddings, sums, counts, self.unseen, self.proto["alpha"], self.proto["min_pixels"])
        seen_e, unseen_e = torch.zeros_like(adapted), torch.zeros_like(adapted)
        seen_e[self.seen] = adapted[self.seen]
        unseen_e[self.unseen] = adapted[self.unseen]
        self._proto_saved = (self.embeddings, self.seen_embeddings, self.unseen_embeddings)
        try:
            self.last_proto = (sums.cpu().numpy(), counts.cpu().numpy())
            if self.rank == 0:
                self._proto_report(self.last_proto[0], self.last_proto[1], shots.cpu().numpy())
            self.embeddings, self.seen_embeddings, self.unseen_embeddings = adapted, seen_e, unseen_e
            yield
        finally:
            self.embeddings, self.seen_embeddings, self.unseen_embeddings = self._proto_saved
            self._proto_saved = None

    def validate(self, both_fcn_and_seenmask=False):
        """reference :182-292.  The {all, seen, unseen} K x K histograms and the loss sum are accumulated on the GPU
        (szn_confusion_hist on the device prediction) and read back ONCE per epoch; under data parallelism the validation
        images are split across the ranks and the histograms / loss sums are all-reduced before the metrics.  With proto= the whole
        validation runs on the adapted class embeddings (adapted_embeddings).  With ema= it runs, prototype pooling included, on the
        averaged weights (engine.TrainStep.averaged_weights); the checkpoint is written after the raw iterate is back in place."""
        step = None
        if self.ema is not None:
            step = self._ema_step()
            self._ema_report(step)
        with (step.averaged_weights() if step is not None else contextlib.nullcontext()):
            with self.adapted_embeddings():
                metrics, is_best = self._validate(both_fcn_and_seenmask)
        self._save_checkpoint(is_best)
        return metrics

    def _ema_report(self, step):
        """once per validation: one ema_log.csv row (rank 0) with the relative L2 distance |avg - w| / |w| of the weight buffer"""
        if self.rank != 0:
            return
        rel = float((torch.linalg.vector_norm(step.ema_w - step.flat_w) / torch.linalg.vector_norm(step.flat_w)).item())
        with open(osp.join(self.log_dir, 'ema_log.csv'), 'a') as f:
            f.write(','.join(map(str, [self.epoch, self.iteration, self.ema["decay"], self.ema["every"], step.ema_updates, rel])) + '\n')
        self.tb_writer.add_scalar('fcn/val/ema_rel_l2_distance', rel, self.epoch)

    def _validate(self, both_fcn_and_seenmask):
        """-> (metrics, whether this validation's mean IU is the best so far)"""
        import torch.distributed as dist
        self.model.eval()
        world = dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1
        hist = torch.zeros(3, self.n_class, self.n_class, dtype=torch.int64, device=self.device)
        acc = torch.zeros(2, dtype=torch.float64, device=self.device)          # loss sum, image-batch count
        if both_fcn_and_seenmask and (self.calibration is not None or self.calib_sweep is not None):
            raise SznError(calibration_refused(True, True, False, True, False, self.n_class))
        if both_fcn_and_seenmask and self.hub is not None:
            raise SznError(hub_refused(True, True, False, True, False, self.n_class))
        if both_fcn_and_seenmask and self.conse is not None:
            raise SznError(conse_refused(True, True, False, True, False, False))
        if not both_fcn_and_seenmask and (self.seen_threshold is not None or self.seen_sweep is not None):
            raise SznError(seen_threshold_refused(True, True, False, False, False, self.n_class))
        if not both_fcn_and_seenmask and self.seen_gate is not None:
            raise SznError(seen_gate_refused(True, True, False, False, False, self.n_class))
        for sweep in self._sweeps:
            if sweep.candidates() is not None:
                sweep.begin()
        n_viz = self.visualize if self.rank == 0 else 0                        # rank 0 renders the first images of its own shard
        tiles = []                                                             # device pictures, kept there until the epoch ends
        mean_bgr = vis_utils.dataset_mean_bgr(getattr(self.val_loader, 'dataset', None)) if n_viz else None
        with torch.no_grad():
            for batch_idx, (data, target) in enumerate(self.val_loader):
                # a loader that is not already sharded per rank (train.py shards it: each rank decodes only its own images)
                if world > 1 and not getattr(self.val_loader, 'szn_sharded', False) and batch_idx % world != self.rank:
                    continue
                score, loss, pred, tgt, img = self._predict_device(data, target, both_fcn_and_seenmask, with_image=True)
                if len(tiles) < n_viz:
                    # reference :198-206, for every image of the batch; no read-back, no host synchronisation
                    viz = vis_utils.visualize_segmentation_device(img, tgt, pred, self.n_class, unseen=self.val_unseen, mean_bgr=mean_bgr)
                    tiles.extend(viz[:n_viz - len(tiles)])
                acc[0] += loss.double()
                acc[1] += 1
                utils.confusion_hist_device(tgt, pred, self.n_class, self.val_unseen if self.unseen else None, hist)
                if self.verbose_val and self.rank == 0:
                    print("Test Epoch {:<5} | Iteration {:<5} | Loss {:5.5f} | Score Sum {:10.5f}".format(
                        int(self.epoch), int(batch_idx), float(loss.item()), float(score.sum().item())))
        if world > 1:
            dist.all_reduce(hist)
            dist.all_reduce(acc)
        calib_hist, seen_hist, conse_hist = (sweep.finish(world) for sweep in self._sweeps)     # collectives: every rank, this order
        h = hist.cpu().numpy()
        if self.rank == 0:
            if self.hub is not None:
                self._hub_report(h, calib_hist)
            elif calib_hist is not None:
                self._calib.report(calib_hist)
            if seen_hist is not None and self.seen_gate is not None:
                self._gate_report(seen_hist)
            elif seen_hist is not None:
                self._seen.report(seen_hist)
            if conse_hist is not None:
                self._conse.report(conse_hist)
        accn = acc.cpu().numpy()
        if np.isnan(accn[0]):
            raise ValueError('loss is nan while validating')
        val_loss = float(accn[0])
        n_batches = max(int(accn[1]), 1)
        metrics = utils._hist_to_metrics(h[0])
        seen_metrics = unseen_metrics = None
        if self.unseen:
            seen_metrics, unseen_metrics = utils._hist_to_metrics(h[1]), utils._hist_to_metrics(h[2])
        val_loss /= n_batches                           # averaged over images like the reference (:246)
        names = ['pxl_acc', 'class_acc', 'mean_iu', 'fwavacc']
        if self.rank == 0:
            with open(osp.join(self.log_dir, 'val_log.csv'), 'a') as f:
                row = [self.epoch, self.iteration, val_loss] + list(metrics)
                if self.unseen:
                    row += list(seen_metrics) + list(unseen_metrics)
                row += [_now() - self.timestamp_start]
                f.write(','.join(map(str, row)) + '\n')
            self.tb_writer.add_scalar('fcn/val/loss', val_loss, self.epoch)
            for grp, ms in (('', metrics), ('seen/', seen_metrics), ('unseen/', unseen_metrics)):
                if ms is None:
                    continue
                for n, v in zip(names, ms):
                    self.tb_writer.add_scalar('fcn/val/%s%s' % (grp, n), v, self.epoch)
                    print('%s%s: %.3f' % ((grp.replace('/', ' ') or 'overall '), n, v))
            if tiles:
                out = osp.join(self.log_dir, 'szn_viz' if both_fcn_and_seenmask else 'fcn_viz')     # reference :209-219
                os.makedirs(out, exist_ok=True)
                self.last_viz = vis_utils.save_mosaic(tiles, osp.join(out, 'epoch%d.jpg' % self.epoch))
                self.tb_writer.add_image('fcn/segmentations', self.last_viz, self.epoch, dataformats='HWC')
        mean_iu = metrics[2]
        is_best = mean_iu > self.best_mean_iu
        if is_best:
            self.best_mean_iu = mean_iu
        return metrics, is_best

    def _save_checkpoint(self, is_best):
        """reference :281-292; with ema= the average rides next to the raw iterate ('model_state_dict' stays the raw iterate)"""
        if self._step is not None:
            self._step.gather_masters()          # sharded optimizer: a collective -- every rank, before rank 0 reads the parameters
        if self.rank == 0:
            if self._step is not None:
                self._step.export_optimizer_state(self.optim)   # flat moments -> per-parameter torch optimizer state
            ckpt = {
                'epoch': self.epoch,
                'iteration': self.iteration,
                'arch': self.model.__class__.__name__,
                'optim_state_dict': self.optim.state_dict(),
                'model_state_dict': self.model.state_dict(),
                'best_mean_iu': self.best_mean_iu,
            }
            if self.ema is not None:
                ckpt['ema_state_dict'] = self._step.ema_state_dict()
                ckpt['ema_updates'] = self._step.ema_updates
            torch.save(ckpt, osp.join(self.log_dir, 'checkpoint'))
            if is_best:
                shutil.copy(osp.join(self.log_dir, 'checkpoint'), osp.join(self.log_dir, 'best'))

    def train(self):
        for epoch in range(self.max_epoch):
            self.epoch = epoch
            if hasattr(getattr(self.train_loader, 'sampler', None), 'set_epoch'):
                self.train_loader.sampler.set_epoch(epoch)       # DistributedSampler: a new shuffle per epoch
            self.train_epoch()
            self.validate()
            # early stop once as many images were seen as in 50 epochs without zero-shot (reference :300-306)
            cur_iter = self.epoch * len(self.train_loader)
            if (self.dataset == 'pascal' and cur_iter > 425000) or (self.dataset == 'context' and cur_iter > 247000):
                break
