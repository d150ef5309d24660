#!/usr/bin/env python
"""train.py -- CLI entry point of the SZN training path (mirrors /root/reference/train.py).

Same flags (-n -g -c -dir -tb -m -d -tu -vu -e -ve -lr -loss -o -se -slr -oh -fu -r; reference :20-42), same
configuration merge / validation (:202-251), same optimizer wiring (two parameter groups, :126-133,302-331) and
two-phase orchestration (FCN phase, then seen-mask phase with the backbone frozen, :161-194).

Added for this implementation (none change the reference flags):
  --synthetic N H W    deterministic synthetic dataset (no PASCAL data / network here); without it the PASCAL-VOC /
                       PASCAL-Context readers of datasets.py load <data_dir> in the reference's layout
  --batch-size B       images per GPU per step (reference: 1)
  --precision fp32|bf16|fp16|bf16x3 (bf16x3: fp32 tensors, conv GEMMs on split-bf16 matrix cores, fp32-accurate)
  --viz N              render the first N validation images per epoch on the GPU into <log_dir>/{fcn,szn,seenmask}_viz/epoch<E>.jpg
                       (vis_utils; 25 = the reference's behaviour, 0 = off)
  --crop-size H W      train on randomly scaled, cropped and mirrored images at a fixed H x W network input (datasets.Augment; one
                       kernel on the GPU, szn_augment_u8); --scale-range LO HI (default 0.5 2.0), --no-flip.  Validation is untouched
  --rotate DEG         with --crop-size: rotate every training image by an angle from [-DEG, DEG]; --color-jitter B C S H: brightness
                       (fraction of 255), contrast, saturation, hue (degrees).  Either switches the augmentation to one affine kernel
                       (szn_augment_affine_u8: a 2 x 3 position map and a 3 x 4 colour matrix per image).  No default strengths
  --conse T            ConSE zero-shot inference for the softmax network (-c 1): validation and -m test_fcn -r <ckpt> mix the class
                       embeddings (--conse-dim E, default 300) of the top T seen classes with their softmax probabilities per pixel and
                       name the nearest class by cosine (szn_conse_head); --conse-gamma G penalises the seen classes, --conse-sweep LO
                       HI N writes the metrics of N penalties to <log_dir>/conse_log.csv from the same head launch
  --calibration GAMMA  calibrated stacking in validation and -m test_fcn: GAMMA is subtracted from the cosine similarity of every seen
                       class before the argmax (szn_calib_head); --calib-sweep LO HI N also writes the metrics of N penalties between
                       LO and HI, and their harmonic mean of seen and unseen mIoU, to <log_dir>/calib_log.csv at one extra head launch
                       per validation batch
  --seen-threshold TAU with -m test_all: a pixel takes the seen class group iff its seen-mask logit margin s1 - s0 exceeds TAU, that
                       is p(seen) > sigmoid(TAU) (szn_seen_sweep_head; 0 = the plain decision); --seen-sweep LO HI N also writes the
                       metrics of N thresholds between LO and HI, and their harmonic mean of seen and unseen mIoU, to
                       <log_dir>/seen_sweep_log.csv from the same head launch
  --seen-gate WEIGHT   with -m test_all: the soft seen/unseen gate p(k|x) = p(group|x) p(k|group,x) (szn_soft_gate_head) -- the cut acts on
                       the margin minus WEIGHT * (log P_U(best unseen) - log P_S(best seen)), the experts' softmaxes over the cosines at
                       --gate-temperature T (default 0.1, a hyper-parameter default, not a tuned value).  0 = the hard cut, 1 = the
                       probabilistic rule.  Composes with --seen-threshold / --seen-sweep; the sweep's rows go to seen_gate_log.csv
  --hub-correct MODE   hubness correction in validation and -m test_fcn (szn_hub_stats, szn_hub_head): per image, every class's mean cosine
                       similarity over the image's pixels is taken off its similarity (mean), and the result divided by the class's
                       spread (zscore), before --calibration's rule (gamma 0 without it); --hub-beta B scales the mean taken off (default
                       1, the textbook form) and --hub-min-sd S floors the spread (default 0.05): defaults nobody has tuned.  Composes
                       with --calibration / --calib-sweep; the rows, with the hubness of each prediction, go to <log_dir>/hub_log.csv
  -loss sim_ce         similarity cross-entropy: softmax over the seen classes' cosine similarities to the pixel embedding, cross
                       entropy against the label (szn_fused_simce_head; the unseen classes do not compete); --sim-temperature T
                       (default 0.1, a hyper-parameter default, not a tuned value) divides the similarities
  -loss rank           hinge ranking loss (DeViSE): a pixel's cosine to its own class embedding must exceed its cosine to every other
                       seen class by a margin (szn_fused_rank_head; the unseen classes are no negatives); --rank-margin M (default 0.1,
                       DeViSE's value: a hyper-parameter default, not a tuned value), --rank-hardest keeps the hardest negative alone
                       instead of the sum of hinges
  --pseudo-label KEEP  self-training on the unseen classes: the training set keeps the images 'train_seen' drops for their unseen classes,
                       with those pixels hidden (--hide-unseen, implied), and every step labels the most confident KEEP (0 < KEEP <= 1) of
                       the hidden pixels per unseen class with its own calibrated prediction (szn_pseudo_head) and trains on them;
                       --pseudo-gamma G (default: --calibration, else 0), --pseudo-floor C (smallest similarity a label may have,
                       default none), --pseudo-start-epoch N (default 0); counts per epoch and class in <log_dir>/pseudo_log.csv
  --bias-loss LAMBDA   with -loss sim_ce: the unseen-bias loss of QFSL on the pixels the training set hides (--hide-unseen, implied): each
                       adds LAMBDA * -log of the probability its softmax over all classes gives the unseen ones
                       (szn_fused_simce_bias_head); no class is committed to.  LAMBDA has no default; --bias-start-epoch N (default 0).
                       Combines with --pseudo-label: relabelled pixels get the supervised term, the still-hidden ones this term
  --ohem KEEP          hard-pixel mining for the embedding losses: every training step trains on the KEEP (0 < KEEP <= 1) of each image's
                       labelled pixels whose cosine to their own class embedding is lowest (szn_ohem_head) and ignores the rest;
                       --ohem-thresh C also keeps every pixel whose cosine lies below C (bins of 1/512), --ohem-start-epoch N
                       (default 0); pixel counts per epoch in <log_dir>/ohem_log.csv.  Validation is never mined
  --proto-shots N      few-shot prototype adaptation of the unseen classes: every validation pools, from N one-class masks per unseen class
                       (datasets.SupportSet over split 'train'), the mean unit vector of the class's pixels (szn_class_proto) with the
                       current weights and evaluates with the class embedding's direction moved --proto-alpha A (default 0.5, the
                       midpoint: a hyper-parameter nobody has tuned) of the way from the word vector to it; --proto-mode unit|raw
                       (default unit), --proto-min-pixels P (default 1); one row per class in <log_dir>/proto_log.csv.  Training never
                       sees the adapted rows
  --ema DECAY          averaged weights (Polyak averaging) for the FCN phase: an fp32 copy of the parameters follows them on the GPU
                       (szn_ema_step, skipped on the device with the steps the fp16 loss scale skips); --ema-every N (default 1),
                       --ema-no-warmup.  Validation and all its logs run on the average (szn_swap_f32 puts it under the model and takes
                       it out again, bit for bit); checkpoints carry 'ema_state_dict' / 'ema_updates' next to the raw iterate and -r
                       restores them; -m test_fcn / test_all --use-ema evaluates the stored average; one row per validation in
                       <log_dir>/ema_log.csv.  DECAY has no default
  --clip-grad-norm MAX clip every step's gradient to the global L2 norm MAX (torch.nn.utils.clip_grad_norm_'s rule) inside the fused
                       step: per-layer sums and sums of squares taken on the GPU after the exchange (szn_grad_stats), the coefficient
                       by szn_clip_coef, the update by the *_clipped optimizer entries; no host sync.  --grad-stats alone measures
                       (MAX = inf).  Either flag: one row per iteration in <log_dir>/grad_log.csv (norm, coefficient, clipped steps,
                       one norm per layer) and score_fr's gradient sum in the progress print.  MAX has no default
  --accum-steps A      gradient accumulation for the FCN phase: A iterations (loader batches) per optimizer step.  The fused step sums its
                       flat gradient buffers on the GPU (szn_grad_accum, left to right like torch's backward() without zero_grad()) and
                       runs exchange, clipping, optimizer and --ema on every A-th iteration only; the update uses the mean of the A
                       gradients (their sum under the pixel-sum cross entropy of -c 1).  Logs stay per iteration, grad_log.csv has one
                       row per optimizer step, a window is carried across epochs, a resumed run restarts its window.  The seen-mask
                       phase runs unaccumulated.  Default: 1
  --init synthetic|vgg path handling: without the caffe VGG16 file the backbone starts from synth weights
  torchrun: RANK / LOCAL_RANK / WORLD_SIZE are honoured (one process per GPU, RCCL gradient all-reduce).
"""
import argparse
import datetime
import os
import os.path as osp

import torch
import torch.nn as nn
import yaml

from . import engine as _engine
from . import models, trainer_fcn, trainer_seenmask
from .configs import configurations
from ._lib import CONSE_MAX_TOP
from .heads import GATE_TEMPERATURE, HUB_BETA, HUB_MIN_SD, RANK_MARGIN, SIM_TEMPERATURE
from .optim import FusedAdam, FusedSGD
from .synthetic_dataset import SyntheticSegmentation


def build_parser():
    p = argparse.ArgumentParser()
    # default value args
    p.add_argument('-n', '--name', type=str, default=None, help='name of checkpoint folder')
    p.add_argument('-g', '--gpu', type=int, default=0, help='gpu number')
    p.add_argument('-c', '--config', type=int, default=1, choices=configurations.keys())
    p.add_argument('-dir', '--data_dir', type=str, default='data', help='path for storing dataset, logs, and models')
    p.add_argument('-tb', '--tb_dir', type=str, default=None, help='path to tensorboard directory (optional)')
    # override cfg args
    p.add_argument('-m', '--mode', type=str, choices=['train', 'test_fcn', 'test_all'])
    p.add_argument('-d', '--dataset', type=str, choices=['pascal', 'context'])
    p.add_argument('-tu', '--train_unseen', type=str, help='comma separated zero-shot train-split unseen classes')
    p.add_argument('-vu', '--val_unseen', type=str, help='comma separated zero-shot val-split unseen classes')
    p.add_argument('-e', '--embed_dim', type=int, choices=[2, 5, 10, 20, 21, 50, 100, 200, 300])
    p.add_argument('-ve', '--fcn_epochs', type=int)
    p.add_argument('-lr', '--fcn_learning_rate', type=float)
    p.add_argument('-loss', '--fcn_loss', type=str, choices=['cos', 'mse', 'sim_ce', 'rank', 'cross_entropy'])
    p.add_argument('-o', '--fcn_optim', type=str, choices=['sgd', 'adam'])
    p.add_argument('-se', '--seenmask_epochs', type=int)
    p.add_argument('-slr', '--seenmask_learning_rate', type=float)
    # optional cfg args
    p.add_argument('-oh', '--one_hot_embed', action='store_true')
    p.add_argument('-fu', '--forced_unseen', action='store_true')
    p.add_argument('-r', '--resume', type=str, help='fcn model checkpoint path')
    # additions
    p.add_argument('--synthetic', type=int, nargs=3, metavar=('N', 'H', 'W'), help='synthetic dataset: N images of HxW')
    p.add_argument('--batch-size', type=int, default=1)
    p.add_argument('--precision', choices=['fp32', 'bf16', 'fp16', 'bf16x3'], default='fp32')
    p.add_argument('--arch', choices=['fcn32s', 'fcn8s'], default='fcn32s',
                   help="fcn32s = the reference's only backbone (train.py:103,105); fcn8s = the public FCN8s skip head "
                        "(not in the reference: BASELINE north_star wording, parity unpinned)")
    p.add_argument('--workers', type=int, default=2, help='DataLoader worker processes per loader (0 = load in the main process)')
    p.add_argument('--viz', type=int, default=0, metavar='N',
                   help="render the first N validation images of every epoch on the GPU and write the mosaic to "
                        "<log_dir>/{fcn_viz,szn_viz,seenmask_viz}/epoch<E>.jpg (and to tensorboard); 25 is the reference's behaviour, "
                        "0 (default) writes nothing")
    p.add_argument('--crop-size', type=int, nargs=2, metavar=('H', 'W'), default=None,
                   help="training augmentation on the GPU: every training image is randomly scaled, cropped to H x W and mirrored, so "
                        "every step runs at one shape (padding carries the ignored label -2); validation is unchanged.  Off by default")
    p.add_argument('--scale-range', type=float, nargs=2, metavar=('LO', 'HI'), default=[0.5, 2.0],
                   help="with --crop-size: the isotropic scale of each image is drawn uniformly from [LO, HI]")
    p.add_argument('--no-flip', action='store_true', help="with --crop-size: never mirror")
    p.add_argument('--rotate', type=float, default=None, metavar='DEG',
                   help="with --crop-size: also rotate every training image about its centre by an angle drawn uniformly from "
                        "[-DEG, DEG] degrees (szn_augment_affine_u8; PSPNet-style pipelines use 10).  No default strength: nobody has "
                        "tuned one here.  Off by default")
    p.add_argument('--color-jitter', type=float, nargs=4, metavar=('B', 'C', 'S', 'H'), default=None,
                   help="with --crop-size: photometric jitter of every training image, each strength >= 0: brightness +-B as a fraction "
                        "of 255, contrast factor in [1-C, 1+C] about the mean colour, saturation factor in [1-S, 1+S], hue +-H degrees "
                        "(one colour matrix per image, szn_augment_affine_u8; SSD-style pipelines use about 0.125 0.5 0.5 18).  No "
                        "default strengths: nobody has tuned them here.  Off by default")
    p.add_argument('--eval-scales', type=float, nargs='+', metavar='S', default=None,
                   help="multi-scale validation (per-epoch validation, -m test_fcn, -m test_all): every image is evaluated at each of "
                        "these scales (1.0 must be among them) and the classes' cosine similarities are summed over the views; "
                        "embedding configurations only.  Default: once, as stored")
    p.add_argument('--eval-flip', action='store_true', help="validation also evaluates the mirror image of every view (alone: of the "
                                                            "stored image)")
    p.add_argument('--calibration', type=float, default=None, metavar='GAMMA',
                   help="calibrated stacking: validation (and -m test_fcn) subtracts GAMMA from the cosine similarity of every seen "
                        "class before the argmax; needs unseen classes and an embedding configuration.  Default: no penalty")
    p.add_argument('--calib-sweep', type=float, nargs=3, metavar=('LO', 'HI', 'N'), default=None,
                   help="every validation also evaluates N penalties (2 to 64) evenly spaced from LO to HI in one extra pass of the "
                        "head and appends their metrics and the harmonic mean of seen and unseen mIoU to <log_dir>/calib_log.csv")
    p.add_argument('--conse', type=int, default=None, metavar='T',
                   help="ConSE zero-shot inference for the softmax network (-c 1: fcn_loss cross_entropy, no embedding): validation "
                        "(and -m test_fcn -r <ckpt>, on any such checkpoint, without retraining) mixes the class embeddings of the top "
                        "T (1 to %d) seen classes with their softmax probabilities per pixel and names the nearest class by cosine "
                        "among all classes; needs unseen classes.  T has no default: nobody has tuned it here (the paper uses 1, 10 "
                        "and 1000).  Default: off" % CONSE_MAX_TOP)
    p.add_argument('--conse-dim', type=int, default=None, choices=[2, 5, 10, 20, 21, 50, 100, 200, 300], metavar='E',
                   help="with --conse: the width of the dataset's class embeddings (default 300)")
    p.add_argument('--conse-gamma', type=float, default=None, metavar='G',
                   help="with --conse: the penalty subtracted from the cosine of every seen class before the two groups are compared "
                        "(calibrated stacking; default 0, at which ConSE almost never names an unseen class)")
    p.add_argument('--conse-sweep', type=float, nargs=3, metavar=('LO', 'HI', 'N'), default=None,
                   help="with --conse: every validation also evaluates N penalties (2 to 64) evenly spaced from LO to HI in the same "
                        "pass of the head and appends their metrics and the harmonic mean of seen and unseen mIoU to "
                        "<log_dir>/conse_log.csv")
    p.add_argument('--seen-threshold', type=float, default=None, metavar='TAU',
                   help="with -m test_all: threshold on the seen-mask logit margin s1 - s0, in logit units -- a pixel is classified "
                        "among the seen classes iff the margin exceeds TAU, that is p(seen) > sigmoid(TAU).  Default: the plain "
                        "decision s1 > s0, which is TAU = 0")
    p.add_argument('--seen-sweep', type=float, nargs=3, metavar=('LO', 'HI', 'N'), default=None,
                   help="with -m test_all: also evaluates N thresholds (2 to 64) evenly spaced from LO to HI in the same pass of the "
                        "head and appends their metrics and the harmonic mean of seen and unseen mIoU to <log_dir>/seen_sweep_log.csv")
    p.add_argument('--hub-correct', choices=('mean', 'zscore'), default=None,
                   help="hubness correction in validation (and -m test_fcn): per image, every class's mean cosine similarity over the "
                        "image's pixels is taken off its similarity before the class is chosen (mean), and the result divided by the "
                        "class's spread over those pixels (zscore).  Composes with --calibration / --calib-sweep (gamma 0 without them); "
                        "the rows, with the hubness (skewness of the per-class prediction counts) of each, go to <log_dir>/hub_log.csv")
    p.add_argument('--hub-beta', type=float, default=None, metavar='B',
                   help="with --hub-correct: the share of the class mean that is taken off.  Default %g, the textbook form: a default "
                        "nobody has tuned.  An error without --hub-correct" % HUB_BETA)
    p.add_argument('--hub-min-sd', type=float, default=None, metavar='S',
                   help="with --hub-correct zscore: the smallest spread a class's similarities are divided by.  Default %g: a default "
                        "nobody has tuned.  An error without --hub-correct" % HUB_MIN_SD)
    p.add_argument('--seen-gate', type=float, default=None, metavar='WEIGHT',
                   help="with -m test_all: soft seen/unseen gating -- p(class) = p(group) * p(class | group) with p(seen) = "
                        "sigmoid(margin - TAU) and a softmax over the cosines inside each class group, which cuts the margin minus WEIGHT * "
                        "(log P_U(best unseen class) - log P_S(best seen class)) at TAU instead of the margin.  0 = the hard cut between "
                        "the two groups' best classes, 1 = the probabilistic rule, larger values trust the class experts more.  No "
                        "default.  With --seen-sweep the rows go to <log_dir>/seen_gate_log.csv")
    p.add_argument('--gate-temperature', type=float, default=None, metavar='T',
                   help="with --seen-gate: the temperature the cosines are divided by in the two class experts' softmaxes.  Default "
                        "%g: a hyper-parameter default, not a tuned value.  An error without --seen-gate" % GATE_TEMPERATURE)
    p.add_argument('--sim-temperature', type=float, default=None, metavar='T',
                   help="with -loss sim_ce (softmax over the seen classes' cosine similarities to the pixel embedding, cross entropy "
                        "against the label): the temperature the similarities are divided by.  Default %g: a hyper-parameter default, "
                        "not a tuned value.  An error without -loss sim_ce" % SIM_TEMPERATURE)
    p.add_argument('--rank-margin', type=float, default=None, metavar='M',
                   help="with -loss rank (hinge ranking loss: the pixel embedding's cosine to its own class must exceed its cosine to "
                        "every other seen class by M): the margin.  Default %g, DeViSE's value: a hyper-parameter default, not a tuned "
                        "value.  An error without -loss rank" % RANK_MARGIN)
    p.add_argument('--rank-hardest', action='store_true',
                   help="with -loss rank: the hardest negative class alone carries the hinge, not the sum over all seen classes.  An "
                        "error without -loss rank")
    p.add_argument('--pseudo-label', type=float, default=None, metavar='KEEP',
                   help="self-training: every training step labels the most confident KEEP (0 < KEEP <= 1) of the hidden pixels per "
                        "unseen class with its own calibrated prediction and trains on them; implies --hide-unseen; needs unseen "
                        "classes and an embedding configuration.  Default: off")
    p.add_argument('--pseudo-gamma', type=float, default=None, metavar='G',
                   help="with --pseudo-label: the seen-class penalty of the labelling rule (default: --calibration, else 0)")
    p.add_argument('--pseudo-floor', type=float, default=None, metavar='C',
                   help="with --pseudo-label: the smallest cosine similarity a pseudo label may have (default: none)")
    p.add_argument('--pseudo-start-epoch', type=int, default=None, metavar='N',
                   help="with --pseudo-label: the first epoch that self-trains (default 0)")
    p.add_argument('--bias-loss', type=float, default=None, metavar='LAMBDA',
                   help="with -loss sim_ce: every hidden pixel adds LAMBDA * -log(probability of the unseen classes under the softmax "
                        "over all classes) to the loss (QFSL's bias loss); implies --hide-unseen; needs unseen classes.  LAMBDA has no "
                        "default: it is a hyper-parameter nobody has tuned here.  An error without -loss sim_ce.  Default: off")
    p.add_argument('--bias-start-epoch', type=int, default=None, metavar='N',
                   help="with --bias-loss: the first epoch that applies the term (default 0)")
    p.add_argument('--ohem', type=float, default=None, metavar='KEEP',
                   help="hard-pixel mining: every training step trains on the KEEP (0 < KEEP <= 1) of each image's labelled pixels whose "
                        "cosine to their own class embedding is lowest and ignores the others; needs an embedding configuration.  KEEP "
                        "has no default: it is a hyper-parameter nobody has tuned here.  Default: off")
    p.add_argument('--ohem-thresh', type=float, default=None, metavar='C',
                   help="with --ohem: also keep every pixel whose own-class cosine lies below C, rounded down to a multiple of 1/512 "
                        "(default: none)")
    p.add_argument('--ohem-start-epoch', type=int, default=None, metavar='N',
                   help="with --ohem: the first epoch that mines (default 0)")
    p.add_argument('--proto-shots', type=int, default=None, metavar='N',
                   help="few-shot prototype adaptation of the unseen classes: every validation pools, from N labelled one-class masks per "
                        "unseen class (the first N images of split 'train' that show it), the mean unit vector the network gives the "
                        "class's pixels, and evaluates with the class embedding moved towards it; needs an embedding configuration and "
                        "unseen classes.  N has no default.  Default: off")
    p.add_argument('--proto-alpha', type=float, default=None, metavar='A',
                   help="with --proto-shots: how far the embedding's direction moves from the word vector (0) to the prototype (1), in "
                        "[0, 1] (default %g: the midpoint, a hyper-parameter nobody has tuned here)" % trainer_fcn.PROTO_ALPHA)
    p.add_argument('--proto-mode', choices=('unit', 'raw'), default=None,
                   help="with --proto-shots: pool the pixels' unit vectors (unit, the mean a cosine classifier wants; default) or the raw "
                        "score vectors (raw)")
    p.add_argument('--proto-min-pixels', type=int, default=None, metavar='P',
                   help="with --proto-shots: a class with fewer than P pooled pixels keeps its word vector (default 1)")
    p.add_argument('--ema', type=float, default=None, metavar='DECAY',
                   help="averaged weights: every training step of the FCN phase moves an fp32 copy of the parameters towards them on the "
                        "GPU (avg = w + D (avg - w), D = min(DECAY, (1 + s) / (10 + s)) after s applied steps); validation, its logs, "
                        "sweeps and pictures run on the average and the checkpoint carries it as 'ema_state_dict' next to the raw "
                        "iterate.  DECAY in [0, 1) has no default: nobody has tuned it here.  Needs a configuration that trains on the "
                        "fused step (-loss cos | mse | sim_ce | rank, or -c 1 cross entropy).  Default: off")
    p.add_argument('--ema-every', type=int, default=None, metavar='N',
                   help="with --ema: update the average every N-th step, with D ^ N (default 1)")
    p.add_argument('--ema-no-warmup', action='store_true', help="with --ema: D = DECAY from the first step on, without the (1 + s) / (10 + s) ramp")
    p.add_argument('--clip-grad-norm', type=float, default=None, metavar='MAX',
                   help="clip the gradient of every training step of the FCN phase to the global L2 norm MAX, coef = min(1, MAX / (norm + "
                        "1e-6)), on the GPU inside the fused step; rank 0 writes one row per iteration to <log_dir>/grad_log.csv.  MAX > 0 "
                        "has no default: nobody has tuned it here.  Needs a configuration that trains on the fused step.  Default: off")
    p.add_argument('--grad-stats', action='store_true',
                   help="the gradient log of --clip-grad-norm without clipping (MAX = inf): grad_log.csv and score_fr's gradient sum in "
                        "the progress print")
    p.add_argument('--accum-steps', type=int, default=None, metavar='A',
                   help="gradient accumulation for the FCN phase: sum the gradients of A iterations (loader batches) on the GPU and run "
                        "exchange, clipping, optimizer and --ema on every A-th one, with the mean of the A gradients (the sum under the "
                        "pixel-sum cross entropy of -c 1).  One iteration stays one loader batch in every log; a window is carried across "
                        "epochs.  Needs a configuration that trains on the fused step; the seen-mask phase runs unaccumulated.  Default: 1")
    p.add_argument('--use-ema', action='store_true',
                   help="with -m test_fcn / -m test_all: evaluate the averaged weights of the checkpoint ('ema_state_dict') instead of the "
                        "raw iterate ('model_state_dict'); an error for a checkpoint written without --ema.  The checkpoint this "
                        "evaluation writes into its own log directory holds the weights it evaluated, the average, as 'model_state_dict'")
    p.add_argument('--hide-unseen', action='store_true',
                   help="the FCN phase trains on every image 'train_seen' would drop for an unseen class as well, with the pixels of "
                        "the unseen classes hidden from every loss and metric (label -3)")
    return p


def update_cfg_with_args(cfg, args):
    """reference :202-230 (truthiness rules kept: 0 cannot override; -se is parsed but never applied)"""
    cfg = dict(cfg)
    for key, val in (('mode', args.mode), ('dataset', args.dataset), ('embed_dim', args.embed_dim),
                     ('fcn_epochs', args.fcn_epochs), ('fcn_lr', args.fcn_learning_rate), ('fcn_loss', args.fcn_loss),
                     ('fcn_optim', args.fcn_optim), ('seenmask_lr', args.seenmask_learning_rate)):
        if val:
            cfg[key] = val
    for key, val in (('train_unseen', args.train_unseen), ('val_unseen', args.val_unseen)):
        if val:
            cfg[key] = [int(item) for item in val.split(',')]
    cfg['one_hot_embed'] = args.one_hot_embed if args.one_hot_embed else cfg.get('one_hot_embed')
    cfg['forced_unseen'] = args.forced_unseen if args.forced_unseen else cfg.get('forced_unseen')
    cfg['load_fcn_path'] = args.resume if args.resume else cfg.get('load_fcn_path')
    return cfg


_EMBED_LOSSES = trainer_fcn._EMBED_LOSSES          # 'cos' | 'mse' | 'sim_ce' | 'rank': the losses of an embedding configuration


# configuration sanity rules (the reference's checks, train.py:232-251, with its messages: the CLI contract): (broken?, message)
_ONE_HOT_WIDTH = {"pascal": 21, "context": 33}      # classes of the dataset = width of a one-hot class embedding
_CFG_RULES = (
    (lambda c: c['one_hot_embed'] and c['embed_dim'] != _ONE_HOT_WIDTH.get(c['dataset'], c['embed_dim']),
     'joint-embedding space must be size of one-hot embedding space'),
    (lambda c: not c['load_fcn_path'] and (c['mode'] in ('test_fcn', 'test_all') or c['fcn_epochs'] < 1),
     'must load model path via -r flag for test mode'),
    (lambda c: c['seenmask_epochs'] > 0 and not c['train_unseen'],
     "can't train the seenmask classifier without train_unseen specified"),
    (lambda c: c['embed_dim'] == 0 and c['fcn_loss'] in _EMBED_LOSSES,
     "invalid loss function because pixel embedding dimensionality not defined"),
)


def validate_cfg(cfg):
    for broken, message in _CFG_RULES:
        if broken(cfg):
            raise Exception(message)


def get_log_dir(model_name, cfg_num, cfg, data_dir, now=None):
    """<data_dir>/logs/<name>CFG_<n>_<KEY>_<value>_..._TIME_<stamp>_ (reference :253-286)"""
    os.makedirs(data_dir, exist_ok=True)
    name = ('%s_' % model_name) if model_name else ''
    name += "CFG_%d_" % int(cfg_num)
    for k, v in cfg.items():
        if k in ['one_hot_embed', 'forced_unseen'] and not v:
            continue
        if k == 'load_fcn_path':
            continue
        if k in ['train_unseen', 'val_unseen']:
            name += '%s_%s_' % (k.upper(), str(bool(v)))
        else:
            name += '%s_%s_' % (k.upper(), str(v))
    now = now or datetime.datetime.now(datetime.timezone(datetime.timedelta(hours=-5)))
    name += 'TIME_%s_' % now.strftime('%Y%m%d-%H%M%S')
    log_dir = osp.join(data_dir, 'logs', name)
    os.makedirs(log_dir, exist_ok=True)
    return log_dir


def output_cfg(cfg, log_dir, writer):
    for k, v in cfg.items():
        print(k, v)
    with open(osp.join(log_dir, 'config.yaml'), 'w') as f:
        yaml.safe_dump(cfg, f, default_flow_style=False)
    if writer is not None:
        writer.add_text("cfg", '\n'.join(['%s: %s' % (k, str(v)) for k, v in cfg.items()]))


def get_parameters(model, bias=False, seenmask=False):
    """reference :302-331: Conv2d weights | Conv2d biases (seenmask layers excluded); ConvTranspose2d weights are the
    frozen bilinear kernels and yield nothing; unknown module types raise."""
    if seenmask:
        for p in model.seenmask_score.parameters():
            yield p
        for p in model.seenmask_upscore.parameters():
            yield p
        return
    skipped = (nn.ReLU, nn.MaxPool2d, nn.Dropout2d, nn.Sequential, models.FCN32s)
    for name, m in model.named_modules():
        if name in ['seenmask_score', 'seenmask_upscore']:
            continue
        if isinstance(m, nn.Conv2d):
            yield m.bias if bias else m.weight
        elif isinstance(m, nn.ConvTranspose2d):
            if bias:
                assert m.bias is None
        elif isinstance(m, skipped):
            continue
        else:
            raise ValueError('Unexpected module: %s' % str(m))


def make_fcn_optimizer(model, cfg):
    """two parameter groups: conv weights, conv biases at 2x lr (SGD: momentum .99, wd 5e-4 on weights only) :126-133"""
    if cfg['fcn_optim'] == "sgd":
        params = [{'params': list(get_parameters(model, bias=False))},
                  {'params': list(get_parameters(model, bias=True)), 'lr': cfg['fcn_lr'] * 2, 'weight_decay': 0}]
        return FusedSGD(params, lr=cfg['fcn_lr'], momentum=.99, weight_decay=0.0005)
    params = [{'params': list(get_parameters(model, bias=False))},
              {'params': list(get_parameters(model, bias=True)), 'lr': cfg['fcn_lr'] * 2}]
    return FusedAdam(params, lr=cfg['fcn_lr'])


def freeze_for_seenmask(model):
    """phase 2: everything frozen except seenmask_score (w, b) and seenmask_upscore (w) (reference :166-171)"""
    for param in model.parameters():
        param.requires_grad = False
    for p in model.seenmask_score.parameters():
        p.requires_grad = True
    for p in model.seenmask_upscore.parameters():
        p.requires_grad = True


def check_precision(precision, cfg):
    """--precision fp16 trains only where loss scaling exists: the fused steps (engine.TrainStep / SeenmaskStep; see
    trainer_fcn.Trainer.train_epoch) -- an embedding configuration with fcn_loss 'cos', 'mse', 'sim_ce' or 'rank', or the softmax
    configuration"""
    fused_cfg = (cfg['fcn_loss'] in _EMBED_LOSSES and cfg['embed_dim']) or (cfg['fcn_loss'] == 'cross_entropy' and not cfg['embed_dim'])
    if precision == 'fp16' and cfg['mode'] == 'train' and cfg['fcn_epochs'] > 0 and not fused_cfg:
        raise Exception("--precision fp16 needs the fused training step: embedding configuration with fcn_loss 'cos', 'mse', 'sim_ce' or 'rank', or "
                        "the softmax configuration (fcn_loss 'cross_entropy', no embedding) (got loss %r, embed_dim %r); use bf16 "
                        "or fp32" % (cfg['fcn_loss'], cfg['embed_dim']))


def check_eval_views(scales, flip, cfg):
    """--eval-scales / --eval-flip: an embedding configuration (the view-ensemble head sums cosine similarities) and 1.0 among the scales"""
    if not scales and not flip:
        return
    if not (cfg['embed_dim'] and cfg['fcn_loss'] in _EMBED_LOSSES):
        raise Exception("--eval-scales / --eval-flip need an embedding configuration with fcn_loss 'cos', 'mse', 'sim_ce' or 'rank' (got loss %r, "
                        "embed_dim %r)" % (cfg['fcn_loss'], cfg['embed_dim']))
    if scales and 1.0 not in [float(s) for s in scales]:
        raise Exception("--eval-scales must contain 1 (got %r)" % (scales,))


def calib_sweep_values(sweep, flag="--calib-sweep"):
    """--calib-sweep LO HI N -> the N float32 penalties numpy.linspace(LO, HI, N), or None without the flag"""
    if sweep is None:
        return None
    import numpy as np
    lo, hi, n = sweep
    if n != int(n) or not 2 <= int(n) <= 64:
        raise Exception("%s: N must be an integer from 2 to 64 (got %r)" % (flag, n))
    if not (np.isfinite([lo, hi]).all() and lo < hi):
        raise Exception("%s: LO < HI, both finite (got %r, %r)" % (flag, lo, hi))
    vals = np.linspace(lo, hi, int(n)).astype(np.float32)
    if not (np.diff(vals) > 0).all():
        raise Exception("%s: %d values between %r and %r are not distinct in float32" % (flag, int(n), lo, hi))
    return vals


def seen_sweep_values(sweep):
    """--seen-sweep LO HI N -> the N float32 thresholds numpy.linspace(LO, HI, N), or None without the flag"""
    return calib_sweep_values(sweep, "--seen-sweep")


def check_seen_threshold(threshold, sweep, cfg, calibration=None, calib_sweep=None, eval_scales=None, eval_flip=False):
    """--seen-threshold / --seen-sweep: -m test_all only, never together with --calibration / --calib-sweep (another class-assignment
    rule, refused under test_all anyway); otherwise trainer_fcn.seen_threshold_refused"""
    if threshold is None and sweep is None:
        return
    seen_sweep_values(sweep)
    if threshold is not None and (threshold != threshold or threshold in (float('inf'), float('-inf'))):
        raise Exception("--seen-threshold: TAU must be finite (got %r)" % (threshold,))
    if calibration is not None or calib_sweep is not None:
        raise Exception("--seen-threshold / --seen-sweep: not together with --calibration / --calib-sweep (two class-assignment rules)")
    n_class = 21 if cfg['dataset'] == 'pascal' else 33
    why = trainer_fcn.seen_threshold_refused(bool(cfg['train_unseen'] or cfg['val_unseen']),
                                             bool(cfg['embed_dim']) and cfg['fcn_loss'] in _EMBED_LOSSES, bool(cfg['forced_unseen']),
                                             cfg['mode'] == 'test_all', bool(eval_scales or eval_flip), n_class,
                                             os.environ.get("SZN_VERBOSE_VAL", "0") == "1")
    if why:
        raise Exception("--seen-threshold / --seen-sweep: " + why)


def check_seen_gate(weight, temperature, cfg, calibration=None, calib_sweep=None, eval_scales=None, eval_flip=False):
    """--seen-gate / --gate-temperature -> the Trainer's seen_gate dict, or None without the flags: the temperature belongs to the gate;
    otherwise check_seen_threshold's rules (trainer_fcn.seen_gate_refused)"""
    if weight is None:
        if temperature is not None:
            raise Exception("--gate-temperature: belongs to --seen-gate, which is off")
        return None
    if not (weight == weight and 0 <= weight < float('inf')):
        raise Exception("--seen-gate: WEIGHT must be finite and >= 0 (got %r)" % (weight,))
    if temperature is not None and not (temperature == temperature and 0 < temperature < float('inf')):
        raise Exception("--gate-temperature: T must be finite and > 0 (got %r)" % (temperature,))
    if calibration is not None or calib_sweep is not None:
        raise Exception("--seen-gate: not together with --calibration / --calib-sweep (two class-assignment rules)")
    n_class = 21 if cfg['dataset'] == 'pascal' else 33
    why = trainer_fcn.seen_gate_refused(bool(cfg['train_unseen'] or cfg['val_unseen']),
                                        bool(cfg['embed_dim']) and cfg['fcn_loss'] in _EMBED_LOSSES, bool(cfg['forced_unseen']),
                                        cfg['mode'] == 'test_all', bool(eval_scales or eval_flip), n_class,
                                        os.environ.get("SZN_VERBOSE_VAL", "0") == "1")
    if why:
        raise Exception("--seen-gate: " + why)
    return dict(weight=weight, temperature=GATE_TEMPERATURE if temperature is None else temperature)


def check_hub(mode, beta, min_sd, cfg, eval_scales=None, eval_flip=False):
    """--hub-correct / --hub-beta / --hub-min-sd -> the Trainer's hub dict, or None without the flags: beta and min_sd belong to the
    correction; otherwise check_calibration's rules (trainer_fcn.hub_refused)"""
    if mode is None:
        if beta is not None or min_sd is not None:
            raise Exception("--hub-beta / --hub-min-sd: belong to --hub-correct, which is off")
        return None
    if beta is not None and not (beta == beta and 0 <= beta < float('inf')):
        raise Exception("--hub-beta: B must be finite and >= 0 (got %r)" % (beta,))
    if min_sd is not None and not (min_sd == min_sd and 0 < min_sd < float('inf')):
        raise Exception("--hub-min-sd: S must be finite and > 0 (got %r)" % (min_sd,))
    n_class = 21 if cfg['dataset'] == 'pascal' else 33
    why = trainer_fcn.hub_refused(bool(cfg['train_unseen'] or cfg['val_unseen']),
                                  bool(cfg['embed_dim']) and cfg['fcn_loss'] in _EMBED_LOSSES, bool(cfg['forced_unseen']),
                                  cfg['mode'] == 'test_all', bool(eval_scales or eval_flip), n_class,
                                  os.environ.get("SZN_VERBOSE_VAL", "0") == "1")
    if why:
        raise Exception("--hub-correct: " + why)
    return dict(mode=mode, beta=HUB_BETA if beta is None else beta, min_sd=HUB_MIN_SD if min_sd is None else min_sd)


def check_calibration(calibration, sweep, cfg, eval_scales=None, eval_flip=False):
    """--calibration / --calib-sweep: unseen classes, an embedding configuration, and none of the other class-assignment rules
    (forced unseen, -m test_all, multi-scale views); more than 256 classes and SZN_VERBOSE_VAL keep the materialised score"""
    if calibration is None and sweep is None:
        return
    calib_sweep_values(sweep)
    if calibration is not None and calibration != calibration or calibration in (float('inf'), float('-inf')):
        raise Exception("--calibration: GAMMA must be finite (got %r)" % (calibration,))
    n_class = 21 if cfg['dataset'] == 'pascal' else 33
    why = trainer_fcn.calibration_refused(bool(cfg['train_unseen'] or cfg['val_unseen']),
                                          bool(cfg['embed_dim']) and cfg['fcn_loss'] in _EMBED_LOSSES, bool(cfg['forced_unseen']),
                                          cfg['mode'] == 'test_all', bool(eval_scales or eval_flip), n_class,
                                          os.environ.get("SZN_VERBOSE_VAL", "0") == "1")
    if why:
        raise Exception("--calibration / --calib-sweep: " + why)


def check_conse(top, dim, gamma, sweep, cfg, eval_scales=None, eval_flip=False):
    """--conse / --conse-dim / --conse-gamma / --conse-sweep: T in [1, CONSE_MAX_TOP], a finite G, the satellites only with --conse;
    unseen classes, the softmax configuration, and none of -m test_all, multi-scale views, or -fu together with a gamma or a sweep
    (trainer_fcn.conse_refused).  -> the Trainer's conse= dict, or None without the flag"""
    if top is None:
        if dim is not None or gamma is not None or sweep is not None:
            raise Exception("--conse-dim / --conse-gamma / --conse-sweep belong to --conse T")
        return None
    if not 1 <= top <= CONSE_MAX_TOP:
        raise Exception("--conse: T must be from 1 to %d (got %r)" % (CONSE_MAX_TOP, top))
    if gamma is not None and (gamma != gamma or gamma in (float('inf'), float('-inf'))):
        raise Exception("--conse-gamma: G must be finite (got %r)" % (gamma,))
    calib_sweep_values(sweep, "--conse-sweep")
    why = trainer_fcn.conse_refused(bool(cfg['train_unseen'] or cfg['val_unseen']),
                                    not cfg['embed_dim'] and cfg['fcn_loss'] == 'cross_entropy', bool(cfg['forced_unseen']),
                                    cfg['mode'] == 'test_all', bool(eval_scales or eval_flip), bool(gamma) or sweep is not None)
    if why:
        raise Exception("--conse: " + why)
    if sweep is not None and os.environ.get("SZN_VERBOSE_VAL", "0") == "1":
        raise Exception("--conse-sweep: SZN_VERBOSE_VAL needs the materialised score, which the fused head never forms")
    if cfg['dataset'] != 'pascal':
        raise Exception("--conse: the softmax network has 21 channels (the reference's -c 1): dataset 'pascal' only (got %r)" % (cfg['dataset'],))
    return dict(top=int(top), dim=300 if dim is None else int(dim), gamma=0.0 if gamma is None else float(gamma))


def check_pseudo(keep, gamma, floor, start_epoch, hide_unseen, cfg):
    """--pseudo-label / --pseudo-gamma / --pseudo-floor / --pseudo-start-epoch / --hide-unseen: KEEP in (0, 1], finite G and C, N >= 0;
    the satellites only with --pseudo-label; unseen classes and an embedding configuration (trainer_fcn.pseudo_refused)"""
    import math
    has_unseen = bool(cfg['train_unseen'] or cfg['val_unseen'])
    if keep is None:
        if gamma is not None or floor is not None or start_epoch is not None:
            raise Exception("--pseudo-gamma / --pseudo-floor / --pseudo-start-epoch need --pseudo-label")
        if hide_unseen and not has_unseen:
            raise Exception("--hide-unseen needs unseen classes (train_unseen / val_unseen)")
        return
    if not 0.0 < keep <= 1.0:
        raise Exception("--pseudo-label: KEEP must lie in (0, 1] (got %r)" % (keep,))
    for name, v in (("--pseudo-gamma", gamma), ("--pseudo-floor", floor)):
        if v is not None and not math.isfinite(v):
            raise Exception("%s must be finite (got %r)" % (name, v))
    if start_epoch is not None and start_epoch < 0:
        raise Exception("--pseudo-start-epoch: N must not be negative (got %r)" % (start_epoch,))
    n_class = 21 if cfg['dataset'] == 'pascal' else 33
    why = trainer_fcn.pseudo_refused(has_unseen, bool(cfg['embed_dim']) and cfg['fcn_loss'] in _EMBED_LOSSES, n_class)
    if why:
        raise Exception("--pseudo-label: " + why)


def check_bias(weight, start_epoch, cfg):
    """--bias-loss / --bias-start-epoch: only with fcn_loss 'sim_ce'; LAMBDA finite and > 0, N >= 0; the satellite only with
    --bias-loss; unseen classes (trainer_fcn.bias_refused)"""
    import math
    if weight is None:
        if start_epoch is not None:
            raise Exception("--bias-start-epoch needs --bias-loss")
        return
    if cfg['fcn_loss'] != 'sim_ce':
        raise Exception("--bias-loss needs -loss sim_ce (got loss %r)" % (cfg['fcn_loss'],))
    if not (math.isfinite(weight) and weight > 0):
        raise Exception("--bias-loss: LAMBDA must be finite and > 0 (got %r)" % (weight,))
    if start_epoch is not None and start_epoch < 0:
        raise Exception("--bias-start-epoch: N must not be negative (got %r)" % (start_epoch,))
    n_class = 21 if cfg['dataset'] == 'pascal' else 33
    why = trainer_fcn.bias_refused(bool(cfg['train_unseen'] or cfg['val_unseen']), bool(cfg['embed_dim']), cfg['fcn_loss'], n_class)
    if why:
        raise Exception("--bias-loss: " + why)


def check_ohem(keep, thresh, start_epoch, cfg):
    """--ohem / --ohem-thresh / --ohem-start-epoch: KEEP in (0, 1], a finite C, N >= 0; the satellites only with --ohem; an embedding
    configuration (trainer_fcn.ohem_refused)"""
    import math
    if keep is None:
        if thresh is not None or start_epoch is not None:
            raise Exception("--ohem-thresh / --ohem-start-epoch need --ohem")
        return
    if not 0.0 < keep <= 1.0:
        raise Exception("--ohem: KEEP must lie in (0, 1] (got %r)" % (keep,))
    if thresh is not None and not math.isfinite(thresh):
        raise Exception("--ohem-thresh must be finite (got %r)" % (thresh,))
    if start_epoch is not None and start_epoch < 0:
        raise Exception("--ohem-start-epoch: N must not be negative (got %r)" % (start_epoch,))
    n_class = 21 if cfg['dataset'] == 'pascal' else 33
    why = trainer_fcn.ohem_refused(bool(cfg['embed_dim']) and cfg['fcn_loss'] in _EMBED_LOSSES, n_class)
    if why:
        raise Exception("--ohem: " + why)


def check_proto(shots, alpha, mode, min_pixels, cfg):
    """--proto-shots / --proto-alpha / --proto-mode / --proto-min-pixels: N >= 1, A in [0, 1], P >= 1; the satellites only with
    --proto-shots; an embedding configuration with unseen classes (trainer_fcn.proto_refused) -> the Trainer's proto dict, or None"""
    if shots is None:
        if alpha is not None or mode is not None or min_pixels is not None:
            raise Exception("--proto-alpha / --proto-mode / --proto-min-pixels need --proto-shots")
        return None
    n_class = 21 if cfg['dataset'] == 'pascal' else 33
    why = trainer_fcn.proto_refused(bool(cfg['train_unseen'] or cfg['val_unseen']),
                                    bool(cfg['embed_dim']) and cfg['fcn_loss'] in _EMBED_LOSSES, n_class, shots)
    if why:
        raise Exception("--proto-shots: " + why)
    if alpha is not None and not 0.0 <= alpha <= 1.0:
        raise Exception("--proto-alpha: A must lie in [0, 1] (got %r)" % (alpha,))
    if min_pixels is not None and min_pixels < 1:
        raise Exception("--proto-min-pixels: P must be at least 1 (got %r)" % (min_pixels,))
    return trainer_fcn.check_proto(dict(shots=shots, alpha=alpha, mode=mode, min_pixels=min_pixels))


def check_ema(decay, every, no_warmup, use_ema, cfg):
    """--ema / --ema-every / --ema-no-warmup / --use-ema: DECAY in [0, 1), N >= 1; the satellites only with --ema; --ema only where the
    FCN phase trains on engine.TrainStep (trainer_fcn.ema_refused), --use-ema only with the test modes -> the Trainer's ema dict, or None"""
    if use_ema and cfg['mode'] not in ('test_fcn', 'test_all'):
        raise Exception("--use-ema evaluates a checkpoint's averaged weights: -m test_fcn / -m test_all only")
    if decay is None:
        if every is not None or no_warmup:
            raise Exception("--ema-every / --ema-no-warmup need --ema")
        return None
    if cfg['mode'] != 'train':
        raise Exception("--ema averages the weights while training (-m train); --use-ema evaluates a stored average")
    if not 0.0 <= decay < 1.0:
        raise Exception("--ema: DECAY must lie in [0, 1) (got %r)" % (decay,))
    if every is not None and every < 1:
        raise Exception("--ema-every: N must be at least 1 (got %r)" % (every,))
    step_cfg = (cfg['fcn_loss'] in _EMBED_LOSSES and cfg['embed_dim']) or (cfg['fcn_loss'] == 'cross_entropy' and not cfg['embed_dim'])
    why = trainer_fcn.ema_refused(bool(step_cfg))
    if why:
        raise trainer_fcn.SznError("--ema: " + why)
    return dict(decay=decay, every=1 if every is None else every, warmup=not no_warmup)


def check_clip(max_norm, grad_stats, cfg):
    """--clip-grad-norm / --grad-stats: MAX > 0 (inf allowed: measure only), and only where the FCN phase trains on engine.TrainStep
    (trainer_fcn.clip_refused) -> the Trainer's (clip_grad_norm, grad_stats)"""
    if max_norm is None and not grad_stats:
        return None, False
    if cfg['mode'] != 'train':
        raise Exception("--clip-grad-norm / --grad-stats act on training steps (-m train)")
    if max_norm is not None and not max_norm > 0.0:
        raise Exception("--clip-grad-norm: MAX must be > 0 (got %r)" % (max_norm,))
    step_cfg = (cfg['fcn_loss'] in _EMBED_LOSSES and cfg['embed_dim']) or (cfg['fcn_loss'] == 'cross_entropy' and not cfg['embed_dim'])
    why = trainer_fcn.clip_refused(bool(step_cfg))
    if why:
        raise trainer_fcn.SznError("--clip-grad-norm / --grad-stats: " + why)
    return max_norm, bool(grad_stats)


def check_accum(steps, cfg):
    """--accum-steps: A >= 1, training only, and only where the FCN phase trains on engine.TrainStep (trainer_fcn.accum_refused) -> the
    Trainer's accum_steps, or None"""
    if steps is None:
        return None
    if cfg['mode'] != 'train':
        raise Exception("--accum-steps acts on training steps (-m train)")
    if steps < 1:
        raise Exception("--accum-steps: A must be at least 1 (got %r)" % (steps,))
    step_cfg = (cfg['fcn_loss'] in _EMBED_LOSSES and cfg['embed_dim']) or (cfg['fcn_loss'] == 'cross_entropy' and not cfg['embed_dim'])
    why = trainer_fcn.accum_refused(bool(step_cfg))
    if why:
        raise trainer_fcn.SznError("--accum-steps: " + why)
    return int(steps)


def check_affine(rotate, color_jitter, crop_size):
    """--rotate / --color-jitter: both act inside the augmentation of --crop-size and are an error without it; strengths >= 0 -> the
    rotate= and jitter= arguments of datasets.Augment (0.0 and None without the flags: the plain scale / crop / flip kernel)"""
    if rotate is None and color_jitter is None:
        return 0.0, None
    if not crop_size:
        raise Exception("--rotate / --color-jitter act inside the training augmentation: they need --crop-size H W")
    if rotate is not None and not rotate >= 0:
        raise Exception("--rotate: DEG must be at least 0 (got %r)" % (rotate,))
    if color_jitter is not None and not all(v >= 0 for v in color_jitter):
        raise Exception("--color-jitter: B C S H must each be at least 0 (got %r)" % (list(color_jitter),))
    jitter = None if color_jitter is None else dict(zip(('brightness', 'contrast', 'saturation', 'hue'), color_jitter))
    return float(rotate or 0.0), jitter


USE_EMA_MISSING = "--use-ema: the checkpoint %s carries no 'ema_state_dict' (it was written without --ema)"


def checkpoint_weights(checkpoint, use_ema, path=''):
    """the state dict a loaded checkpoint hands the model: the raw iterate, or with --use-ema its averaged weights"""
    if not use_ema:
        return checkpoint['model_state_dict']
    if 'ema_state_dict' not in checkpoint:
        raise Exception(USE_EMA_MISSING % path)
    return checkpoint['ema_state_dict']


def check_sim_temperature(temperature, cfg):
    """--sim-temperature: only with fcn_loss 'sim_ce', positive and finite"""
    if temperature is None:
        return
    if cfg['fcn_loss'] != 'sim_ce':
        raise Exception("--sim-temperature needs -loss sim_ce (got loss %r)" % (cfg['fcn_loss'],))
    if not 0 < temperature < float('inf'):
        raise Exception("--sim-temperature: T must be positive and finite (got %r)" % (temperature,))


def check_rank(margin, hardest, cfg):
    """--rank-margin / --rank-hardest: only with fcn_loss 'rank'; the margin finite and >= 0"""
    if margin is None and not hardest:
        return
    if cfg['fcn_loss'] != 'rank':
        raise Exception("--rank-margin / --rank-hardest need -loss rank (got loss %r)" % (cfg['fcn_loss'],))
    if margin is not None and not 0 <= margin < float('inf'):
        raise Exception("--rank-margin: M must be finite and >= 0 (got %r)" % (margin,))


def main(argv=None):
    args = build_parser().parse_args(argv)
    cfg = update_cfg_with_args(configurations[args.config], args)
    validate_cfg(cfg)
    check_sim_temperature(args.sim_temperature, cfg)
    check_rank(args.rank_margin, args.rank_hardest, cfg)
    check_precision(args.precision, cfg)
    check_eval_views(args.eval_scales, args.eval_flip, cfg)
    check_calibration(args.calibration, args.calib_sweep, cfg, args.eval_scales, args.eval_flip)
    check_seen_threshold(args.seen_threshold, args.seen_sweep, cfg, args.calibration, args.calib_sweep, args.eval_scales, args.eval_flip)
    seen_gate = check_seen_gate(args.seen_gate, args.gate_temperature, cfg, args.calibration, args.calib_sweep, args.eval_scales, args.eval_flip)
    hub = check_hub(args.hub_correct, args.hub_beta, args.hub_min_sd, cfg, args.eval_scales, args.eval_flip)
    conse = check_conse(args.conse, args.conse_dim, args.conse_gamma, args.conse_sweep, cfg, args.eval_scales, args.eval_flip)
    check_pseudo(args.pseudo_label, args.pseudo_gamma, args.pseudo_floor, args.pseudo_start_epoch, args.hide_unseen, cfg)
    check_ohem(args.ohem, args.ohem_thresh, args.ohem_start_epoch, cfg)
    check_bias(args.bias_loss, args.bias_start_epoch, cfg)
    proto = check_proto(args.proto_shots, args.proto_alpha, args.proto_mode, args.proto_min_pixels, cfg)
    ema = check_ema(args.ema, args.ema_every, args.ema_no_warmup, args.use_ema, cfg)
    clip_grad_norm, grad_stats = check_clip(args.clip_grad_norm, args.grad_stats, cfg)
    accum_steps = check_accum(args.accum_steps, cfg)
    rotate, jitter = check_affine(args.rotate, args.color_jitter, args.crop_size)
    hide_unseen = args.hide_unseen or args.pseudo_label is not None or args.bias_loss is not None
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(args.gpu)))
    one_gpu = os.environ.get("SZN_TEST_ONE_GPU") == "1"       # test hook: every rank on device 0 over gloo (1-GPU boxes)
    if one_gpu:
        local_rank = 0
    if not torch.cuda.is_available():
        raise RuntimeError("no GPU visible: this implementation has no CPU path")
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    import torch.distributed as dist
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if one_gpu:
            dist.init_process_group("gloo")
        else:
            _engine.init_process_group("nccl", device)      # RCCL on a high-priority stream (engine.init_process_group)
    torch.manual_seed(1337)
    torch.cuda.manual_seed(1337)

    # one log directory for the whole job: rank 0 stamps it (wall clock), the others receive the name
    log_dir = get_log_dir(args.name, args.config, cfg, args.data_dir) if rank == 0 else None
    if world > 1:
        box = [log_dir]
        dist.broadcast_object_list(box, src=0)
        log_dir = box[0]
    tb_writer = None
    if args.tb_dir and rank == 0:
        try:
            from tensorboardX import SummaryWriter
            tb_writer = SummaryWriter(osp.join(args.tb_dir, log_dir.split('/')[-1]))
        except ImportError:
            print("tensorboardX not installed: tensorboard logging disabled")
    if rank == 0:
        output_cfg(cfg, log_dir, tb_writer)

    # 1. dataset
    all_unseen = cfg['train_unseen'] + cfg['val_unseen']
    collate = None
    augment, train_collate = None, None
    if args.crop_size:
        # the training loaders hand out raw padded batches with their sizes (at every batch size, 1 included); the trainers scale,
        # crop and mirror them on the GPU
        from .datasets import Augment, augment_collate
        augment = Augment(crop=args.crop_size, scale=args.scale_range, flip=not args.no_flip, seed=1337, rotate=rotate, jitter=jitter)
        train_collate = augment_collate
    if args.synthetic:
        n_img, H, W = args.synthetic
        n_class = 21 if cfg['dataset'] == 'pascal' else 33
        mk = lambda split, unseen, n: SyntheticSegmentation(split=split, n_images=n, size=(H, W), n_class=n_class,
                                                             embed_dim=cfg['embed_dim'], unseen=unseen, seed=1337,
                                                             native=augment is not None and split != 'val',
                                                             hide_unseen=hide_unseen and split == 'train_seen')
        # splits as in the reference (pascal_dataset.py:62-74, context_dataset.py:75-94): 'train' drops every image that
        # contains a val_unseen class, 'train_seen' additionally drops the train_unseen classes, 'val' keeps everything
        train_dataset = mk('train', cfg['val_unseen'], n_img)
        train_seen_dataset = mk('train_seen', all_unseen, n_img)
        val_dataset = mk('val', [], max(n_img // 4, 1))
    else:
        # real data under <data_dir> (reference layout, train.py:64-80); samples travel raw (uint8 image + label), the BGR /
        # mean transform and the target-embedding gather run on the GPU; images differ in size: batches > 1 are padded to the
        # largest image of the batch with ignored (-1) pixels (datasets.pad_collate; the reference trains at batch size 1)
        from .datasets import PascalContext, PascalVOC, pad_collate
        if args.batch_size > 1:
            collate = pad_collate
        cls = PascalVOC if cfg['dataset'] == 'pascal' else PascalContext
        mkr = lambda split: cls(split=split, embed_dim=cfg['embed_dim'], one_hot_embed=cfg['one_hot_embed'],
                                data_dir=args.data_dir, train_unseen=cfg['train_unseen'], val_unseen=cfg['val_unseen'],
                                native=True, hide_unseen=hide_unseen and split == 'train_seen')
        train_dataset, train_seen_dataset, val_dataset = mkr('train'), mkr('train_seen'), mkr('val')
    kwargs = {'num_workers': args.workers, 'pin_memory': True}

    def loader(ds, bs, shuffle):
        kw = dict(kwargs, collate_fn=collate) if (collate is not None and bs > 1) else kwargs
        if train_collate is not None and shuffle:          # the two training loaders
            kw = dict(kwargs, collate_fn=train_collate)
        if world > 1 and shuffle:       # every rank holds the same dataset; the sampler deals disjoint shards per epoch
            sampler = torch.utils.data.distributed.DistributedSampler(ds, num_replicas=world, rank=rank, shuffle=True, seed=1337)
            return torch.utils.data.DataLoader(ds, batch_size=bs, sampler=sampler, **kw)
        if world > 1:                   # validation: rank r evaluates images r, r + world, ... and loads ONLY those
            ds = torch.utils.data.Subset(ds, list(range(rank, len(ds), world)))
        return torch.utils.data.DataLoader(ds, batch_size=bs, shuffle=shuffle, **kw)
    train_loader = loader(train_dataset, args.batch_size, True)
    train_seen_loader = loader(train_seen_dataset, args.batch_size, True)
    val_loader = loader(val_dataset, 1, False)            # sharded by rank above; Trainer.validate all-reduces the sums
    val_loader.szn_sharded = world > 1                    # tells the trainers not to skip batches by index on top of it
    label_names = train_dataset.class_names
    support_loader = None
    if proto is not None:
        # the strict K-shot support set: one-class masks of the unseen classes from a 'train' split that shows every class.  Every
        # rank pools the whole (small) set itself: the loader is not sharded
        from .datasets import SupportSet
        if args.synthetic:
            support_base = SyntheticSegmentation(split='train', n_images=n_img, size=(H, W), n_class=n_class,
                                                 embed_dim=cfg['embed_dim'], unseen=[], seed=1337)
        else:
            support_base = cls(split='train', embed_dim=cfg['embed_dim'], one_hot_embed=cfg['one_hot_embed'], data_dir=args.data_dir,
                               train_unseen=[], val_unseen=[], native=True)
        support_loader = torch.utils.data.DataLoader(SupportSet(support_base, all_unseen, proto['shots']), batch_size=1, shuffle=False,
                                                     **kwargs)
    if rank == 0 and not osp.exists(osp.join(log_dir, 'counts.csv')):
        with open(osp.join(log_dir, 'counts.csv'), 'w') as f:
            f.write('train_seen,train_unseen,val\n%d,%d,%d\n' % (len(train_seen_loader), len(train_loader) - len(train_seen_loader),
                                                                 len(val_dataset)))

    # 2. model
    model = {'fcn32s': models.FCN32s, 'fcn8s': models.FCN8s}[args.arch](n_class=cfg['embed_dim'] if cfg['embed_dim'] else 21)
    start_epoch, start_iteration, checkpoint = 0, 0, None
    if cfg['load_fcn_path']:
        checkpoint = torch.load(osp.join(args.data_dir, 'logs', cfg['load_fcn_path'], 'best'), map_location='cpu', weights_only=False)
        model.load_state_dict(checkpoint_weights(checkpoint, args.use_ema, cfg['load_fcn_path']), strict=False)
        start_epoch, start_iteration = checkpoint['epoch'], checkpoint['iteration']
    else:
        try:
            model.copy_params_from_vgg16(models.VGG16(pretrained=True, data_dir=args.data_dir))
        except IOError as e:
            print("%s -> deterministic synthetic initialisation" % e)
            model.load_synthetic(1337)
    model = model.to(device)
    precision = {'bf16': torch.bfloat16, 'fp16': torch.float16, 'fp32': torch.float32, 'bf16x3': 'bf16x3'}[args.precision]
    model.set_precision(precision)
    model._engine.dropout_seed = 1337 + 7919 * rank       # data-parallel ranks draw different Dropout2d masks

    # 3. fcn optimizer and trainer
    optim = make_fcn_optimizer(model, cfg)
    if cfg['load_fcn_path'] and checkpoint.get('optim_state_dict'):
        optim.load_state_dict(checkpoint['optim_state_dict'])
    fcn_trainer = trainer_fcn.Trainer(
        cuda=True, model=model, optimizer=optim, train_loader=train_seen_loader, val_loader=val_loader, log_dir=log_dir,
        dataset=cfg['dataset'], max_epoch=cfg['fcn_epochs'], pixel_embeddings=cfg['embed_dim'], loss_func=cfg['fcn_loss'],
        tb_writer=tb_writer, unseen=all_unseen, val_unseen=cfg['val_unseen'], label_names=label_names,
        forced_unseen=cfg['forced_unseen'], precision=precision, rank=rank, visualize=args.viz, augment=augment,
        proto=proto, support_loader=support_loader,
        seen_threshold=args.seen_threshold, seen_sweep=seen_sweep_values(args.seen_sweep), seen_gate=seen_gate,
        sim_temperature=args.sim_temperature,
        rank_margin=args.rank_margin, rank_hardest=args.rank_hardest,
        pseudo=None if args.pseudo_label is None else dict(keep=args.pseudo_label, gamma=args.pseudo_gamma,
                                                           conf_floor=-2.0 if args.pseudo_floor is None else args.pseudo_floor),
        pseudo_start_epoch=args.pseudo_start_epoch or 0,
        ohem=None if args.ohem is None else dict(keep=args.ohem, thresh=args.ohem_thresh), ohem_start_epoch=args.ohem_start_epoch or 0,
        calibration=args.calibration, calib_sweep=calib_sweep_values(args.calib_sweep), eval_scales=args.eval_scales,
        eval_flip=args.eval_flip, bias_loss=args.bias_loss, bias_start_epoch=args.bias_start_epoch or 0,
        conse=conse, conse_sweep=calib_sweep_values(args.conse_sweep, "--conse-sweep"), hub=hub, ema=ema, ema_checkpoint=checkpoint, clip_grad_norm=clip_grad_norm,
        grad_stats=grad_stats, accum_steps=accum_steps)
    fcn_trainer.epoch, fcn_trainer.iteration = start_epoch, start_iteration

    if cfg['mode'] == 'train':
        if cfg['fcn_epochs'] > 0:
            fcn_trainer.train()
        # 4. seen-mask phase
        if cfg['seenmask_epochs'] > 0:
            freeze_for_seenmask(model)
            sm_optim = FusedAdam([{'params': list(get_parameters(model, seenmask=True))}], lr=cfg['seenmask_lr'])
            if world > 1:
                dist.barrier()               # rank 0 has finished writing <log_dir>/best before anyone reads it
            if not checkpoint:
                # the reference reloads <log_dir>/best (train.py:177-179); fall back to the last checkpoint when no
                # validation improved on best_mean_iu = 0 (tiny synthetic runs)
                for fname in ('best', 'checkpoint'):
                    if osp.exists(osp.join(log_dir, fname)):
                        checkpoint = torch.load(osp.join(log_dir, fname), map_location='cpu', weights_only=False)
                        break
                else:
                    checkpoint = {}
            seenmask_trainer = trainer_seenmask.Trainer(
                cuda=True, model=model, optimizer=sm_optim, train_loader=train_loader, val_loader=val_loader,
                log_dir=log_dir, dataset=cfg['dataset'], max_epoch=cfg['seenmask_epochs'], tb_writer=tb_writer,
                checkpoint=checkpoint, unseen=cfg['train_unseen'], rank=rank, visualize=args.viz,
                augment=augment)
            seenmask_trainer.train()
    elif cfg['mode'] == 'test_fcn':
        fcn_trainer.validate(both_fcn_and_seenmask=False)
    elif cfg['mode'] == 'test_all':
        fcn_trainer.validate(both_fcn_and_seenmask=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
