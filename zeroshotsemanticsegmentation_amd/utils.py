"""utils.py -- losses, nearest-class-embedding inference and segmentation metrics of the SZN path.

Mirrors the function surface of /root/reference/utils.py (same names, argument meaning and return types);
the arithmetic runs in hand-written HIP kernels (csrc/szn_head.hip) through the C-ABI of include/szn.h.
There is no CPU fallback: tensors must live on the GPU.

  load_obj / save_obj                      utils.py:11-17
  cross_entropy2d(score, target, ...)      utils.py:19-48
  mse_loss / cosine_loss                   utils.py:50-102
  sim_ce_loss                              similarity cross-entropy in torch ops (no reference counterpart)
  sim_ce_bias_loss                         sim_ce plus QFSL's unseen-bias term on hidden pixels, in torch ops (no reference counterpart)
  rank_loss                                hinge ranking loss (DeViSE) in torch ops (no reference counterpart)
  label_accuracy_score                     utils.py:104-154
  infer_lbl / infer_lbl_forced_unseen / infer_lbl_szn / stich_seen_unseen_with_mask   utils.py:159-205

Batched semantics (the reference raises for n > 1 in cosine_loss / infer_lbl): per-image loss, mean over
images; inference is applied per image and returns (B,H,W).
"""
import ctypes as C
import pickle

import numpy as np
import torch

from . import _lib as L


def load_obj(name):
    with open(name + '.pkl', 'rb') as f:
        return pickle.load(f, encoding='latin-1')


def save_obj(obj, name):
    with open(name + '.pkl', 'wb') as f:
        pickle.dump(obj, f, pickle.HIGHEST_PROTOCOL)


MEAN_BGR = (104.00698793, 116.66876762, 122.67891434)          # context_dataset.py:51, pascal_dataset.py:41


def image_to_device(img_u8, device=None, mean_bgr=MEAN_BGR):
    """dataset transform on the GPU (context_dataset.py:143-150): uint8 RGB image(s) (H,W,3) or (B,H,W,3) -- host or device --
    -> (B,3,H,W) f32 BGR minus mean_bgr.  The host sends 3 bytes per pixel instead of 12; results are bit-identical to the
    reference's float64 subtraction + .float()."""
    t = img_u8 if isinstance(img_u8, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(img_u8))
    if t.dtype != torch.uint8 or t.shape[-1] != 3 or t.dim() not in (3, 4):
        raise L.SznError("image_to_device expects uint8 (H,W,3) or (B,H,W,3), got %s %s" % (t.dtype, tuple(t.shape)))
    if t.dim() == 3:
        t = t.unsqueeze(0)
    dev = torch.device(device) if device is not None else (t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    t = t.to(dev, non_blocking=True).contiguous()
    B, H, W, _ = t.shape
    out = torch.empty(B, 3, H, W, device=dev, dtype=torch.float32)
    mean = (C.c_double * 3)(*[float(m) for m in mean_bgr])
    L.call("szn_image_u8_to_bgr_f32", B, H, W, L.ptr(t), mean, L.ptr(out), L.stream_ptr())
    return out


def augment_to_device(img_u8, label, params, out_hw, device=None, mean_bgr=MEAN_BGR):
    """training augmentation on the GPU (szn_augment_u8 in include/szn.h; no reference counterpart): the uint8 RGB canvases
    (B,Hm,Wm,3) and labels (B,Hm,Wm) of a padded batch -- host or device -- and one int32 record per image (B, AUG_NPARAM), as
    datasets.Augment.params draws them -> (data (B,3,Ho,Wo) f32 BGR minus mean_bgr, target (B,Ho,Wo) int64), each image randomly
    scaled, cropped to out_hw and mirrored; pixels outside the scaled image are 0.0 / datasets.PAD_LABEL."""
    return _augment("augment_to_device", "szn_augment_u8", L.AUG_NPARAM, img_u8, label, params, out_hw, device, mean_bgr)


def augment_affine_to_device(img_u8, label, params, out_hw, device=None, mean_bgr=MEAN_BGR):
    """augment_to_device with rotation and colour jitter (szn_augment_affine_u8 in include/szn.h): the same inputs and outputs, the
    records are the (B, AUGA_NPARAM) int32 affine ones -- a 2 x 3 fixed-point position map and a 3 x 4 fixed-point colour matrix per
    image, as datasets.Augment.params draws them with rotate / jitter set."""
    return _augment("augment_affine_to_device", "szn_augment_affine_u8", L.AUGA_NPARAM, img_u8, label, params, out_hw, device, mean_bgr)


def _augment(who, entry, nparam, img_u8, label, params, out_hw, device, mean_bgr):
    as_t = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    t, lbl, rec = as_t(img_u8), as_t(label), as_t(params)
    if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[-1] != 3:
        raise L.SznError("%s expects uint8 (B,Hm,Wm,3) images, got %s %s" % (who, t.dtype, tuple(t.shape)))
    B, Hm, Wm, _ = t.shape
    if tuple(lbl.shape) != (B, Hm, Wm) or lbl.is_floating_point():
        raise L.SznError("%s expects integer (B,Hm,Wm) labels matching the images, got %s %s" % (who, lbl.dtype, tuple(lbl.shape)))
    if rec.dtype != torch.int32 or tuple(rec.shape) != (B, nparam):
        raise L.SznError("%s expects int32 (%d,%d) params, got %s %s" % (who, B, nparam, rec.dtype, tuple(rec.shape)))
    Ho, Wo = int(out_hw[0]), int(out_hw[1])
    dev = torch.device(device) if device is not None else (t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    t = t.to(dev, non_blocking=True).contiguous()
    lbl = lbl.to(device=dev, dtype=torch.int64, non_blocking=True).contiguous()
    rec = rec.to(dev, non_blocking=True).contiguous()
    data = torch.empty(B, 3, max(Ho, 0), max(Wo, 0), device=dev, dtype=torch.float32)
    target = torch.empty(B, max(Ho, 0), max(Wo, 0), device=dev, dtype=torch.int64)
    mean = (C.c_double * 3)(*[float(m) for m in mean_bgr])
    L.call(entry, B, Hm, Wm, L.ptr(t), L.ptr(lbl), L.ptr(rec), mean, Ho, Wo, L.ptr(data), L.ptr(target), L.stream_ptr())
    return data, target


def _need_cuda(t, what):
    if not t.is_cuda:
        raise L.SznError("%s must be a GPU tensor (the HIP path has no CPU fallback)" % what)


def _prep(score, target):
    _need_cuda(score, "score")
    score = score.contiguous().float()
    target = target.to(device=score.device, dtype=torch.int64).contiguous()
    return score, target


class _EmbedLoss(torch.autograd.Function):
    """cosine (mode 'cos') / mse (mode 'mse') loss against a per-pixel target embedding"""

    @staticmethod
    def forward(ctx, score, target, table, dense, mode):
        B, E, H, W = score.shape
        dev = score.device
        loss = torch.empty(1, device=dev)
        stats = torch.empty(B, 2, device=dev)
        ws = torch.empty(L.load().szn_loss_workspace_bytes(B, H, W), dtype=torch.uint8, device=dev)
        K = 0 if table is None else table.shape[0]
        fn = "szn_cosine_loss_fwd" if mode == "cos" else "szn_mse_loss_fwd"
        L.call(fn, B, E, H, W, K, L.ptr(score), L.ptr(target), L.ptr(table), L.ptr(dense), L.ptr(loss), L.ptr(stats),
               L.ptr(ws), L.stream_ptr())
        ctx.save_for_backward(score, target, stats)
        ctx.table, ctx.dense, ctx.mode = table, dense, mode
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gout):
        score, target, stats = ctx.saved_tensors
        B, E, H, W = score.shape
        dscore = torch.empty_like(score)
        g = gout.contiguous().float().reshape(1)
        table, dense = ctx.table, ctx.dense
        K = 0 if table is None else table.shape[0]
        fn = "szn_cosine_loss_bwd" if ctx.mode == "cos" else "szn_mse_loss_bwd"
        L.call(fn, B, E, H, W, K, L.ptr(score), L.ptr(target), L.ptr(table), L.ptr(dense), L.ptr(stats), L.ptr(g),
               L.ptr(dscore), L.stream_ptr())
        return dscore, None, None, None, None


def _embed_loss(score, target, target_embed, mode):
    score, target = _prep(score, target)
    te = target_embed.detach() if isinstance(target_embed, torch.Tensor) else torch.as_tensor(target_embed)
    te = te.to(device=score.device, dtype=torch.float32).contiguous()
    if te.dim() == 2:            # (K,E) class-embedding matrix: gather rows by label on the device
        if te.shape[1] != score.shape[1]:
            raise L.SznError("embedding matrix has E=%d, score has %d channels" % (te.shape[1], score.shape[1]))
        return _EmbedLoss.apply(score, target, te, None, mode)
    if te.shape != score.shape:
        raise L.SznError("target_embed shape %s != score shape %s" % (tuple(te.shape), tuple(score.shape)))
    return _EmbedLoss.apply(score, target, None, te, mode)


def cosine_loss(score, target, target_embed):
    """Negative cosine similarity loss (reference utils.py:75-102).

    score (n,c,h,w); target (n,h,w) with -1 = ignore; target_embed (n,c,h,w) as in the reference, OR the
    (K,c) class-embedding matrix, in which case the per-pixel target vector is gathered by label on the GPU
    (ignore pixels are masked either way)."""
    return _embed_loss(score, target, target_embed, "cos")


def mse_loss(score, target, target_embed):
    """Masked sum of squared differences / number of valid pixels (reference utils.py:50-73)."""
    return _embed_loss(score, target, target_embed, "mse")


def sim_ce_loss(score, target, embed, exclude=None, temperature=0.1):
    """Similarity cross-entropy (include/szn.h, szn_fused_simce_head): per pixel the cross entropy of softmax_k(cos(s, e_k) / T) over
    the classes k NOT in `exclude` against the label; labels < 0, >= K or in `exclude` are ignored; per image the sum of the terms
    over its counted pixels, the loss is the mean over images.  Plain differentiable torch ops on the materialised score (n,c,h,w), in
    the score's own dtype (float32 or float64) and on its device: the autograd route and the in-suite referee of the fused head.
    embed: the (K,c) class-embedding matrix; a zero row counts with norm 1."""
    if score.dim() != 4:
        raise L.SznError("sim_ce_loss: score must be (n,c,h,w), got %s" % (tuple(score.shape),))
    if not float(temperature) > 0 or not np.isfinite(float(temperature)):
        raise L.SznError("sim_ce_loss: temperature must be positive and finite, got %r" % (temperature,))
    B, E, H, W = score.shape
    emb = torch.as_tensor(embed).detach().to(device=score.device, dtype=score.dtype)
    K = emb.shape[0]
    if emb.dim() != 2 or emb.shape[1] != E:
        raise L.SznError("sim_ce_loss: embedding matrix %s does not match the score's %d channels" % (tuple(emb.shape), E))
    excl = sorted(set(int(k) for k in (exclude if exclude is not None else [])))
    if any(not 0 <= k < K for k in excl):
        raise L.SznError("sim_ce_loss: exclude names a class outside [0, %d)" % K)
    if len(excl) >= K:
        raise L.SznError("sim_ce_loss: exclude leaves no class competing")
    competes = torch.ones(K, dtype=torch.bool, device=score.device)
    if excl:
        competes[torch.tensor(excl, device=score.device)] = False
    target = target.to(device=score.device, dtype=torch.int64)
    en = emb.norm(dim=1)
    en = torch.where(en == 0, torch.ones_like(en), en)
    s = score.permute(0, 2, 3, 1)                                        # (B,H,W,E)
    cos = (s @ emb.t()) / (s.norm(dim=3, keepdim=True) * en)             # (B,H,W,K)
    zall = cos / float(temperature)
    z = zall.masked_fill(~competes, float("-inf"))
    in_range = (target >= 0) & (target < K)
    lbl = torch.where(in_range, target, torch.zeros_like(target))
    counted = in_range & competes[lbl]
    term = torch.logsumexp(z, dim=3) - zall.gather(3, lbl.unsqueeze(3)).squeeze(3)
    term = torch.where(counted, term, torch.zeros_like(term))
    per_image = term.sum(dim=(1, 2)) / counted.sum(dim=(1, 2)).to(score.dtype)
    return per_image.mean()


def sim_ce_bias_loss(score, target, embed, exclude=None, temperature=0.1, unseen=(), weight=1.0, hidden_label=-3):
    """sim_ce_loss plus QFSL's unseen-bias term (include/szn.h, szn_fused_simce_bias_head): a labelled pixel (0 <= label < K, label not
    in `exclude`) has sim_ce_loss's term; a pixel labelled `hidden_label` has weight * -log sum_{u in unseen} softmax_u(cos(s, e_k) / T)
    with the softmax over ALL K classes, formed as logsumexp_all - logsumexp_unseen so that it stays finite where the unseen
    probability itself underflows; every other pixel is ignored.  Per image the sum of all terms over the number of labelled plus hidden
    pixels (one joint mean), the loss is the mean over images.  Plain differentiable torch ops on the materialised score (n,c,h,w), in
    the score's own dtype (float32 or float64) and on its device: the autograd route and the in-suite referee of the fused head.
    hidden_label: datasets.HIDDEN_LABEL by default (datasets imports this module, hence the literal)."""
    if score.dim() != 4:
        raise L.SznError("sim_ce_bias_loss: score must be (n,c,h,w), got %s" % (tuple(score.shape),))
    if not float(temperature) > 0 or not np.isfinite(float(temperature)):
        raise L.SznError("sim_ce_bias_loss: temperature must be positive and finite, got %r" % (temperature,))
    if not float(weight) > 0 or not np.isfinite(float(weight)):
        raise L.SznError("sim_ce_bias_loss: weight must be positive and finite, got %r" % (weight,))
    if int(hidden_label) >= -1:
        raise L.SznError("sim_ce_bias_loss: the hidden label must lie below -1, got %r" % (hidden_label,))
    B, E, H, W = score.shape
    emb = torch.as_tensor(embed).detach().to(device=score.device, dtype=score.dtype)
    K = emb.shape[0]
    if emb.dim() != 2 or emb.shape[1] != E:
        raise L.SznError("sim_ce_bias_loss: embedding matrix %s does not match the score's %d channels" % (tuple(emb.shape), E))
    excl = sorted(set(int(k) for k in (exclude if exclude is not None else [])))
    if any(not 0 <= k < K for k in excl):
        raise L.SznError("sim_ce_bias_loss: exclude names a class outside [0, %d)" % K)
    if len(excl) >= K:
        raise L.SznError("sim_ce_bias_loss: exclude leaves no class competing")
    uns = sorted(set(int(k) for k in unseen))
    if not uns or uns[0] < 0 or uns[-1] >= K or len(uns) >= K:
        raise L.SznError("sim_ce_bias_loss: unseen must name some, not all, classes of [0, %d)" % K)
    competes = torch.ones(K, dtype=torch.bool, device=score.device)
    if excl:
        competes[torch.tensor(excl, device=score.device)] = False
    in_u = torch.zeros(K, dtype=torch.bool, device=score.device)
    in_u[torch.tensor(uns, device=score.device)] = True
    target = target.to(device=score.device, dtype=torch.int64)
    en = emb.norm(dim=1)
    en = torch.where(en == 0, torch.ones_like(en), en)
    s = score.permute(0, 2, 3, 1)                                        # (B,H,W,E)
    cos = (s @ emb.t()) / (s.norm(dim=3, keepdim=True) * en)             # (B,H,W,K)
    zall = cos / float(temperature)
    in_range = (target >= 0) & (target < K)
    lbl = torch.where(in_range, target, torch.zeros_like(target))
    labelled = in_range & competes[lbl]
    hidden = target == int(hidden_label)
    sup = torch.logsumexp(zall.masked_fill(~competes, float("-inf")), dim=3) - zall.gather(3, lbl.unsqueeze(3)).squeeze(3)
    bias = float(weight) * (torch.logsumexp(zall, dim=3) - torch.logsumexp(zall.masked_fill(~in_u, float("-inf")), dim=3))
    term = torch.where(labelled, sup, torch.where(hidden, bias, torch.zeros_like(sup)))
    per_image = term.sum(dim=(1, 2)) / (labelled | hidden).sum(dim=(1, 2)).to(score.dtype)
    return per_image.mean()


def rank_loss(score, target, embed, exclude=None, margin=0.1, hardest=False):
    """Hinge ranking loss (include/szn.h, szn_fused_rank_head; DeViSE): per pixel sum_k max(0, margin - cos(s, e_label) + cos(s, e_k))
    over the classes k != label NOT in `exclude` -- with `hardest` the largest of these hinges alone (the lowest class index on an
    exact tie); labels < 0, >= K or in `exclude` are ignored; per image the sum of the terms over its counted pixels divided by
    their number, the loss is the mean over images.  Plain differentiable torch ops on the materialised score (n,c,h,w), in the score's
    own dtype (float32 or float64) and on its device: the autograd route and the in-suite referee of the fused head.
    embed: the (K,c) class-embedding matrix; a zero row counts with norm 1."""
    if score.dim() != 4:
        raise L.SznError("rank_loss: score must be (n,c,h,w), got %s" % (tuple(score.shape),))
    if not float(margin) >= 0 or not np.isfinite(float(margin)):
        raise L.SznError("rank_loss: margin must be finite and >= 0, got %r" % (margin,))
    B, E, H, W = score.shape
    emb = torch.as_tensor(embed).detach().to(device=score.device, dtype=score.dtype)
    K = emb.shape[0]
    if emb.dim() != 2 or emb.shape[1] != E:
        raise L.SznError("rank_loss: embedding matrix %s does not match the score's %d channels" % (tuple(emb.shape), E))
    excl = sorted(set(int(k) for k in (exclude if exclude is not None else [])))
    if any(not 0 <= k < K for k in excl):
        raise L.SznError("rank_loss: exclude names a class outside [0, %d)" % K)
    if K - len(excl) < 2:
        raise L.SznError("rank_loss: exclude leaves fewer than two classes competing")
    competes = torch.ones(K, dtype=torch.bool, device=score.device)
    if excl:
        competes[torch.tensor(excl, device=score.device)] = False
    target = target.to(device=score.device, dtype=torch.int64)
    en = emb.norm(dim=1)
    en = torch.where(en == 0, torch.ones_like(en), en)
    s = score.permute(0, 2, 3, 1)                                        # (B,H,W,E)
    cos = (s @ emb.t()) / (s.norm(dim=3, keepdim=True) * en)             # (B,H,W,K)
    in_range = (target >= 0) & (target < K)
    lbl = torch.where(in_range, target, torch.zeros_like(target))
    counted = in_range & competes[lbl]
    v = float(margin) - cos.gather(3, lbl.unsqueeze(3)) + cos            # (B,H,W,K)
    negative = competes.expand_as(v).clone()
    negative.scatter_(3, lbl.unsqueeze(3), False)                        # the label is no negative of its own pixel
    if hardest:
        # max() sends the gradient to the first maximal index: the lowest class index on a tie
        term = v.masked_fill(~negative, float("-inf")).max(dim=3)[0].clamp(min=0)
    else:
        term = torch.where(negative, v, torch.zeros_like(v)).clamp(min=0).sum(dim=3)
    term = torch.where(counted, term, torch.zeros_like(term))
    per_image = term.sum(dim=(1, 2)) / counted.sum(dim=(1, 2)).to(score.dtype)
    return per_image.mean()


class _CE2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, score, target, size_average, weight):
        B, Cc, H, W = score.shape
        dev = score.device
        loss = torch.empty(1, device=dev)
        stats = torch.empty(B, 2, device=dev)
        ws = torch.empty(L.load().szn_loss_workspace_bytes(B, H, W), dtype=torch.uint8, device=dev)
        L.call("szn_ce2d_fwd", B, Cc, H, W, L.ptr(score), L.ptr(target), L.ptr(weight), int(size_average), L.ptr(loss),
               L.ptr(stats), None, L.ptr(ws), L.stream_ptr())
        ctx.save_for_backward(score, target, stats)
        ctx.size_average, ctx.weight = size_average, weight
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gout):
        score, target, stats = ctx.saved_tensors
        B, Cc, H, W = score.shape
        dscore = torch.empty_like(score)
        g = gout.contiguous().float().reshape(1)
        L.call("szn_ce2d_bwd", B, Cc, H, W, L.ptr(score), L.ptr(target), L.ptr(ctx.weight), int(ctx.size_average), L.ptr(stats),
               L.ptr(g), L.ptr(dscore), L.stream_ptr())
        return dscore, None, None, None


def cross_entropy2d(score, target, weight=None, size_average=False):
    """log-softmax over channels + masked, optionally class-weighted NLL sum, optionally / #valid pixels (reference
    utils.py:19-48; `weight` = the (C,) tensor handed to F.nll_loss at utils.py:46; size_average divides by the number of
    valid pixels, not by the weight sum, utils.py:47-48)."""
    score, target = _prep(score, target)
    if weight is not None:
        weight = torch.as_tensor(weight).detach().to(device=score.device, dtype=torch.float32).contiguous()
        if weight.dim() != 1 or weight.numel() != score.shape[1]:
            raise L.SznError("cross_entropy2d: weight must have one entry per class (%d), got %s"
                             % (score.shape[1], tuple(weight.shape)))
    return _CE2d.apply(score, target, bool(size_average), weight)


def channel_argmax(score):
    """score.data.max(1)[1] (trainer_fcn.py:117, trainer_seenmask.py:67) -> int64 (B,H,W) device tensor"""
    _need_cuda(score, "score")
    score = score.detach().contiguous().float()
    B, Cc, H, W = score.shape
    dev = score.device
    pred = torch.empty(B, H, W, dtype=torch.int64, device=dev)
    dummy_t = torch.full((B, H, W), -1, dtype=torch.int64, device=dev)
    loss = torch.empty(1, device=dev); stats = torch.empty(B, 2, device=dev)
    ws = torch.empty(L.load().szn_loss_workspace_bytes(B, H, W), dtype=torch.uint8, device=dev)
    L.call("szn_ce2d_fwd", B, Cc, H, W, L.ptr(score), L.ptr(dummy_t), None, 0, L.ptr(loss), L.ptr(stats), L.ptr(pred), L.ptr(ws),
           L.stream_ptr())
    return pred


# ---- nearest-neighbouring-embedding inference --------------------------------------------------------------
def _data(t):
    return t.data if isinstance(t, torch.Tensor) else torch.as_tensor(t)


def infer_lbl_device(score, embed_arr, mode=0, unseen=None, seenmask=None, target=None):
    """int64 (B,H,W) DEVICE tensor; see szn_embed_argmax in include/szn.h"""
    score = _data(score)
    _need_cuda(score, "score")
    score = score.contiguous().float()
    emb = _data(embed_arr).to(device=score.device, dtype=torch.float32).contiguous()
    B, E, H, W = score.shape
    if emb.dim() != 2 or emb.shape[1] != E:
        raise L.SznError("embed_arr must be (K,%d), got %s" % (E, tuple(emb.shape)))
    pred = torch.empty(B, H, W, dtype=torch.int64, device=score.device)
    sm = None if seenmask is None else _data(seenmask).to(score.device).contiguous().float()
    tg = None if target is None else _data(target).to(device=score.device, dtype=torch.int64).contiguous()
    L.call("szn_embed_argmax_k", B, E, H, W, emb.shape[0], L.ptr(score), L.ptr(emb), mode,
           L.class_set(unseen), L.ptr(sm), L.ptr(tg), L.ptr(pred), L.stream_ptr())
    return pred


def infer_lbl(score, embed_arr, cuda=False):
    """argmax_k cos(score_px, embed_k), zero-norm rows score 0 and still compete (reference utils.py:159-185).
    Returns numpy int64 (n,h,w)."""
    return infer_lbl_device(score, embed_arr).cpu().numpy()


def _split_unseen(seen_embed_arr, unseen_embed_arr):
    """recover (full matrix, unseen class list) from the zero-masked pair built at trainer_fcn.py:56-64"""
    se, ue = _data(seen_embed_arr).float(), _data(unseen_embed_arr).float()
    unseen = torch.nonzero(ue.abs().sum(1) > 0).flatten().tolist()
    return se + ue, unseen


def stich_seen_unseen_with_mask(score, seen_embed_arr, unseen_embed_arr, unseen_mask, cuda):
    """reference utils.py:201-205 with an explicit boolean mask (numpy or tensor, (n,h,w))"""
    full, unseen = _split_unseen(seen_embed_arr, unseen_embed_arr)
    dev = _data(score).device
    m = torch.as_tensor(np.asarray(unseen_mask)).to(dev)
    # encode the mask as a 2-channel "seenmask score": channel 1 > channel 0 <=> seen
    sm = torch.stack([m.float(), 1.0 - m.float()], 1)
    return infer_lbl_device(score, full, mode=1, unseen=unseen, seenmask=sm).cpu().numpy()


def infer_lbl_forced_unseen(score, target, seen_embed_arr, unseen_embed_arr, unseen, cuda=False):
    """seen pixels choose among seen classes, GT-unseen pixels among unseen classes (reference utils.py:188-192)"""
    full, _ = _split_unseen(seen_embed_arr, unseen_embed_arr)
    return infer_lbl_device(score, full, mode=1, unseen=unseen, target=target).cpu().numpy()


def infer_lbl_szn(score, seen_mask_score, seen_embed_arr, unseen_embed_arr, cuda=False):
    """full SZN inference: the 2-channel seen-mask argmax picks the group (reference utils.py:195-199)"""
    full, unseen = _split_unseen(seen_embed_arr, unseen_embed_arr)
    return infer_lbl_device(score, full, mode=1, unseen=unseen, seenmask=seen_mask_score).cpu().numpy()


# ---- metrics -----------------------------------------------------------------------------------------------
def confusion_hist_device(label_true, label_pred, n_class, unseen=None, hist=None):
    """accumulate the {all, seen, unseen} K x K histograms on the GPU (reference utils.py:104-119,138-152)"""
    lt = _data(label_true)
    _need_cuda(lt, "label_true")
    lt = lt.to(torch.int64).contiguous()
    lp = _data(label_pred).to(device=lt.device, dtype=torch.int64).contiguous()
    if hist is None:
        hist = torch.zeros(3, n_class, n_class, dtype=torch.int64, device=lt.device)
    L.call("szn_confusion_hist_k", lt.numel(), n_class, L.ptr(lt), L.ptr(lp), L.class_set(unseen), L.ptr(hist),
           L.stream_ptr())
    return hist


def _hist_to_metrics(hist):
    """acc, mean class acc, mean IU, fw IU with the reference's nan-mean rules (utils.py:121-129)"""
    hist = np.asarray(hist, dtype=np.float64)
    with np.errstate(all="ignore"):
        acc = np.diag(hist).sum() / hist.sum()
        acc_cls = np.nanmean(np.diag(hist) / hist.sum(axis=1))
        iu = np.diag(hist) / (hist.sum(axis=1) + hist.sum(axis=0) - np.diag(hist))
        mean_iu = np.nanmean(iu)
        freq = hist.sum(axis=1) / hist.sum()
        fwavacc = (freq[freq > 0] * iu[freq > 0]).sum()
    return acc, acc_cls, mean_iu, fwavacc


def harmonic_mean_iu(seen_metrics, unseen_metrics):
    """the generalized zero-shot score: the harmonic mean 2 s u / (s + u) of the seen and the unseen mean IU (the mean_iu entries of
    two _hist_to_metrics tuples).  0.0 when s + u == 0, NaN when either is NaN."""
    s, u = float(seen_metrics[2]), float(unseen_metrics[2])
    if np.isnan(s) or np.isnan(u):
        return float('nan')
    if s + u == 0:
        return 0.0
    return 2.0 * s * u / (s + u)


def blend_prototypes(embeddings, sums, counts, classes, alpha, min_pixels=1):
    """few-shot adaptation of class embeddings: move the rows `classes` of `embeddings` (K,E) from their word vector towards the class
    prototype sums[k] (heads.class_proto / FCN32s.class_prototypes: the sum of the class's pixel vectors; only its direction matters).
    For each k in `classes` with counts[k][1] >= min_pixels, |sums[k]| != 0 and |e_k| != 0:
        d = (1 - alpha) e_k / |e_k| + alpha sums[k] / |sums[k]|,     row k = |e_k| d / |d|       (float64; the row keeps its norm, so the
    norm-sensitive losses validation reports stay comparable); the row stays when d = 0.  Every other row is the input's, bit for bit,
    and alpha = 0 returns the input bit for bit.  -> a new (K,E) float32 tensor (on the device of `embeddings` when that is a tensor)."""
    alpha = float(alpha)
    if not 0.0 <= alpha <= 1.0:
        raise L.SznError("blend_prototypes: alpha must lie in [0, 1], got %r" % (alpha,))
    dev = embeddings.device if isinstance(embeddings, torch.Tensor) else None
    e32 = np.array(_data(embeddings).detach().cpu().numpy() if isinstance(embeddings, torch.Tensor) else embeddings, dtype=np.float32)
    s = np.asarray(sums.detach().cpu().numpy() if isinstance(sums, torch.Tensor) else sums, dtype=np.float64)
    c = np.asarray(counts.detach().cpu().numpy() if isinstance(counts, torch.Tensor) else counts, dtype=np.int64)
    K, E = e32.shape
    if s.shape != (K, E) or c.shape != (K, 2):
        raise L.SznError("blend_prototypes: sums %r / counts %r do not fit embeddings %r" % (s.shape, c.shape, e32.shape))
    out = e32.copy()
    for k in sorted(set(int(k) for k in classes)):
        if not 0 <= k < K:
            raise L.SznError("blend_prototypes: class %d outside [0, %d)" % (k, K))
        e = e32[k].astype(np.float64)
        en, sn = np.sqrt((e * e).sum()), np.sqrt((s[k] * s[k]).sum())
        if alpha == 0.0 or c[k, 1] < int(min_pixels) or not (np.isfinite(sn) and sn > 0.0 and en > 0.0):
            continue
        d = (1.0 - alpha) * (e / en) + alpha * (s[k] / sn)
        dn = np.sqrt((d * d).sum())
        if dn > 0.0:
            out[k] = (en * (d / dn)).astype(np.float32)
    t = torch.from_numpy(out)
    return t if dev is None else t.to(dev)


def calib_rows(hist, n_class, unseen):
    """one gamma's (K,K) confusion histogram -> (metrics, seen metrics, unseen metrics): the seen / unseen histograms are its rows
    with the target outside / inside `unseen`, the others zero (what szn_confusion_hist_k fills)"""
    hist = np.asarray(hist)
    is_unseen = np.zeros(n_class, dtype=bool)
    is_unseen[list(unseen)] = True
    seen_h = np.where(is_unseen[:, None], 0, hist)
    unseen_h = np.where(is_unseen[:, None], hist, 0)
    return _hist_to_metrics(hist), _hist_to_metrics(seen_h), _hist_to_metrics(unseen_h)


def _first_max(vals, members):
    """(class, value) of the first class of `members` (ascending) holding the maximum of vals (B,K,H,W) over them"""
    sub = vals[:, members]
    best = sub.max(dim=1, keepdim=True).values
    pos = torch.arange(len(members), device=vals.device).view(1, -1, 1, 1)
    first = torch.where(sub == best, pos, len(members)).min(dim=1).values.clamp(max=len(members) - 1)
    return members[first], best[:, 0]


def conse_infer(score, embeddings, unseen, top_t, gamma=0.0, target=None):
    """ConSE (Norouzi et al., ICLR 2014) on a materialised (B,K,H,W) softmax-network score with torch operations: the referee of
    szn_conse_head (heads.conse, FCN32s.conse_predict) and the route for configurations the fused head does not take (more than 256
    classes, SZN_VERBOSE_VAL).  Runs on the score's device, CPU included.  Per pixel: the top `top_t` SEEN classes (not in `unseen`)
    by (score descending, class ascending), their softmax p, the mixture f = sum p_t e_t of the rows of `embeddings` (K,E), the cosine
    of f with every row (a zero norm counts as 1); a / b = the first best seen / unseen class, m = their cosine difference.
    target None: a where m > gamma, or m == gamma and a < b; else b (0 where m is NaN).  target given: the reference's forced rule
    -- b where the target names an unseen class, a elsewhere; gamma is not used.  -> int64 (B,H,W) tensor on the score's device."""
    score = _data(score).detach().float()
    dev = score.device
    emb = _data(embeddings).to(device=dev, dtype=torch.float32)
    B, K, H, W = score.shape
    if emb.dim() != 2 or emb.shape[0] != K:
        raise L.SznError("conse_infer: embeddings must be (%d,E), got %s" % (K, tuple(emb.shape)))
    uns = sorted(set(int(k) for k in unseen))
    if not uns or len(uns) >= K or uns[0] < 0 or uns[-1] >= K:
        raise L.SznError("conse_infer: the unseen classes must be a non-empty proper subset of range(%d)" % K)
    if int(top_t) < 1:
        raise L.SznError("conse_infer: top_t must be at least 1, got %r" % (top_t,))
    is_unseen = torch.zeros(K, dtype=torch.bool, device=dev)
    is_unseen[uns] = True
    seen_idx, unseen_idx = torch.nonzero(~is_unseen)[:, 0], torch.nonzero(is_unseen)[:, 0]
    n = min(int(top_t), int(seen_idx.numel()))
    vals, order = torch.sort(score[:, seen_idx], dim=1, descending=True, stable=True)       # stable: ties keep the class order
    p = torch.softmax(vals[:, :n], dim=1)
    probs = torch.zeros_like(score).scatter_(1, seen_idx[order[:, :n]], p)                   # (B,K,H,W), zero outside S
    f = torch.einsum('bkhw,ke->behw', probs, emb)
    fn = f.norm(dim=1, keepdim=True)
    en = emb.norm(dim=1)
    sim = torch.einsum('behw,ke->bkhw', f, emb) / (torch.where(fn == 0, torch.ones_like(fn), fn)
                                                   * torch.where(en == 0, torch.ones_like(en), en).view(1, K, 1, 1))
    a, va = _first_max(sim, seen_idx)
    b, vb = _first_max(sim, unseen_idx)
    m = va - vb
    if target is not None:
        tgt = _data(target).to(device=dev, dtype=torch.int64)
        pred = torch.where(torch.isin(tgt, unseen_idx), b, a)
    else:
        g = float(np.float32(gamma))
        pred = torch.where((m > g) | ((m == g) & (a < b)), a, b)
    return torch.where(torch.isnan(m), torch.zeros_like(pred), pred)


def soft_gate_infer(score, seen_mask_score, embeddings, unseen, tau, temperature, weight):
    """the soft seen/unseen gate on a materialised (B,E,H,W) embedding score and (B,2,H,W) seen-mask score with torch operations: the
    referee of szn_soft_gate_head (heads.soft_gate, FCN32s.seen_gate_predict).  Runs on the score's device, CPU included.  Per pixel:
    the cosine of the score with every row of `embeddings` (K,E) (a zero-norm pixel: NaN); a / b = the first best seen / unseen class;
    l_S = log sum_{k seen} exp((cos_k - cos_a) / temperature) = -log P_S(a), l_U likewise; e = (s1 - s0) - weight * (l_S - l_U).
    a where e > tau, else b (a NaN margin: b); class 0 where l_S - l_U is NaN.  -> int64 (B,H,W) tensor on the score's device."""
    score = _data(score).detach().float()
    dev = score.device
    sm = _data(seen_mask_score).detach().to(device=dev, dtype=torch.float32)
    emb = _data(embeddings).to(device=dev, dtype=torch.float32)
    K = emb.shape[0]
    if emb.dim() != 2 or emb.shape[1] != score.shape[1]:
        raise L.SznError("soft_gate_infer: embeddings must be (K,%d), got %s" % (score.shape[1], tuple(emb.shape)))
    uns = sorted(set(int(k) for k in unseen))
    if not uns or len(uns) >= K or uns[0] < 0 or uns[-1] >= K:
        raise L.SznError("soft_gate_infer: the unseen classes must be a non-empty proper subset of range(%d)" % K)
    t, w = float(np.float32(temperature)), float(np.float32(weight))
    if not (np.isfinite(t) and t > 0 and np.isfinite(w) and w >= 0):
        raise L.SznError("soft_gate_infer: temperature must be finite and > 0, weight finite and >= 0")
    is_unseen = torch.zeros(K, dtype=torch.bool, device=dev)
    is_unseen[uns] = True
    seen_idx, unseen_idx = torch.nonzero(~is_unseen)[:, 0], torch.nonzero(is_unseen)[:, 0]
    sim = torch.einsum('behw,ke->bkhw', score, emb) / (score.norm(dim=1, keepdim=True) * emb.norm(dim=1).view(1, K, 1, 1))
    a, va = _first_max(sim, seen_idx)
    b, vb = _first_max(sim, unseen_idx)
    ls = torch.log(torch.exp((sim[:, seen_idx] - va.unsqueeze(1)) / t).sum(dim=1))
    lu = torch.log(torch.exp((sim[:, unseen_idx] - vb.unsqueeze(1)) / t).sum(dim=1))
    d = ls - lu
    e = (sm[:, 1] - sm[:, 0]) - w * d
    pred = torch.where(e > float(np.float32(tau)), a, b)
    return torch.where(torch.isnan(d), torch.zeros_like(pred), pred)


def hub_infer(score, embeddings, unseen, mode, beta, gamma=0.0, min_sd=0.05, valid=None):
    """hubness-corrected class assignment on a materialised (B,E,H,W) embedding score with torch operations: the referee of szn_hub_stats
    + szn_hub_head (heads.hub_stats, heads.hub, FCN32s.hub_predict).  Runs on the score's device, CPU included.  Per pixel the cosine of
    the score with every row of `embeddings` (K,E) (a zero-norm pixel: NaN); per image and class the mean and the standard deviation
    (population form) of that cosine over the image's pixels with a finite norm > 0 -- and valid (B,H,W) bool where given (False: a padding
    pixel) -- as plain floating means, no quantisation.  mode 'mean': adj = cos - beta * mean; 'zscore': adj = (cos - beta * mean) /
    max(sd, min_sd).  An image without such a pixel keeps its cosines.  a / b = the first best seen / unseen class by adj, m = their
    difference: a where m > gamma, or m == gamma and a < b; else b; class 0 where m is NaN.  -> int64 (B,H,W) tensor on the score's device."""
    score = _data(score).detach().float()
    dev = score.device
    emb = _data(embeddings).to(device=dev, dtype=torch.float32)
    K = emb.shape[0]
    if emb.dim() != 2 or emb.shape[1] != score.shape[1]:
        raise L.SznError("hub_infer: embeddings must be (K,%d), got %s" % (score.shape[1], tuple(emb.shape)))
    uns = sorted(set(int(k) for k in unseen))
    if not uns or len(uns) >= K or uns[0] < 0 or uns[-1] >= K:
        raise L.SznError("hub_infer: the unseen classes must be a non-empty proper subset of range(%d)" % K)
    if mode not in L.HUB_MODES:
        raise L.SznError("hub_infer: mode must be one of %s, got %r" % (sorted(L.HUB_MODES), mode))
    bt, ms = float(np.float32(beta)), float(np.float32(min_sd))
    if not (np.isfinite(bt) and bt >= 0 and np.isfinite(ms) and ms > 0):
        raise L.SznError("hub_infer: beta must be finite and >= 0, min_sd finite and > 0")
    is_unseen = torch.zeros(K, dtype=torch.bool, device=dev)
    is_unseen[uns] = True
    seen_idx, unseen_idx = torch.nonzero(~is_unseen)[:, 0], torch.nonzero(is_unseen)[:, 0]
    sn = score.norm(dim=1, keepdim=True)
    en = emb.norm(dim=1)
    sim = torch.einsum('behw,ke->bkhw', score, emb) / (sn * torch.where(en == 0, torch.ones_like(en), en).view(1, K, 1, 1))
    counted = torch.isfinite(sn) & (sn > 0)
    if valid is not None:
        counted = counted & _data(valid).to(device=dev, dtype=torch.bool).unsqueeze(1)
    n = counted.sum(dim=(2, 3), keepdim=True).to(torch.float32)
    s0 = torch.where(counted, sim, torch.zeros_like(sim))
    n1 = n.clamp(min=1)
    mean = s0.sum(dim=(2, 3), keepdim=True) / n1
    var = ((s0 * s0).sum(dim=(2, 3), keepdim=True) / n1 - mean * mean).clamp(min=0)
    scale = torch.ones_like(mean) if mode == "mean" else 1.0 / var.sqrt().clamp(min=ms)
    some = n > 0
    scale = torch.where(some, scale, torch.ones_like(scale))
    shift = torch.where(some, bt * mean * scale, torch.zeros_like(mean))
    adj = sim * scale - shift
    a, va = _first_max(adj, seen_idx)
    b, vb = _first_max(adj, unseen_idx)
    m = va - vb
    g = float(np.float32(gamma))
    pred = torch.where((m > g) | ((m == g) & (a < b)), a, b)
    return torch.where(torch.isnan(m), torch.zeros_like(pred), pred)


def hubness_skew(hist):
    """the hubness of a prediction: the skewness of N_k, the number of pixels each class was predicted for (the column sums of a (K,K)
    confusion histogram, or the (K,) counts themselves) -- E[(N_k - mu)^3] / sigma^3 over the classes, population moments (Radovanovic et
    al. 2010).  Large and positive: a few classes take most pixels.  0.0 when every class has the same count."""
    h = np.asarray(hist, dtype=np.float64)
    nk = h.sum(axis=0) if h.ndim == 2 else h.reshape(-1)
    d = nk - nk.mean()
    var = (d * d).mean()
    if not var > 0:
        return 0.0
    return float((d ** 3).mean() / var ** 1.5)


def _fast_hist(label_true, label_pred, n_class, target='all', unseen=None):
    """host restatement of utils.py:104-119 for numpy label maps (validation logs on the host)"""
    label_true = np.asarray(label_true)
    label_pred = np.asarray(label_pred)
    mask = (label_true >= 0) & (label_true < n_class)
    if target == 'unseen':
        mask = mask & np.isin(label_true, list(unseen))
    elif target == 'seen':
        mask = mask & np.isin(label_true, [x for x in range(n_class) if x not in unseen])
    return np.bincount(n_class * label_true[mask].astype(int) + label_pred[mask],
                       minlength=n_class ** 2).reshape(n_class, n_class)


def label_accuracy_score(label_trues, label_preds, n_class, unseen=None):
    """overall acc, mean acc, mean IU, fwavacc -- and the same for seen / unseen GT pixels when `unseen` is given
    (reference utils.py:131-154).  Accepts numpy label maps (host) or GPU tensors (histogram on the device)."""
    first = label_trues[0] if isinstance(label_trues, (list, tuple)) else label_trues
    if isinstance(first, torch.Tensor) and first.is_cuda:
        hist = torch.zeros(3, n_class, n_class, dtype=torch.int64, device=first.device)
        lts = label_trues if isinstance(label_trues, (list, tuple)) else [label_trues]
        lps = label_preds if isinstance(label_preds, (list, tuple)) else [label_preds]
        for lt, lp in zip(lts, lps):
            confusion_hist_device(lt, lp, n_class, unseen, hist)
        h = hist.cpu().numpy()
    else:
        h = np.zeros((3, n_class, n_class))
        for lt, lp in zip(label_trues, label_preds):
            lt, lp = np.asarray(lt).flatten(), np.asarray(lp).flatten()
            h[0] += _fast_hist(lt, lp, n_class)
            if unseen:
                h[1] += _fast_hist(lt, lp, n_class, 'seen', unseen)
                h[2] += _fast_hist(lt, lp, n_class, 'unseen', unseen)
    metrics = _hist_to_metrics(h[0])
    if unseen:
        return metrics, _hist_to_metrics(h[1]), _hist_to_metrics(h[2])
    return metrics
