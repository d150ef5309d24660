"""engine.py -- the fused training step of the SZN path (what bench.py measures and the trainers run).

One `TrainStep.step(x, target)` is the reference's hot loop body (trainer_fcn.py:149-180):
    forward (models.py:114-160, train mode)  ->  cosine loss (utils.py:75-102)  ->  train-time
    infer_lbl (utils.py:159-185)  ->  backward  ->  [gradient all-reduce over RCCL]  ->  Adam / SGD step
    (train.py:126-133)  ->  confusion histogram for the running metrics (utils.py:104-154)
without autograd bookkeeping: parameters, gradients and optimizer moments live in flat fp32 buffers (the
module's Parameters are channels_last views into them), the head runs fused from the 1/32 map
(szn_fused_head) and the per-layer gradient buckets are all-reduced on RCCL's stream while the rest of the
backward pass is still running.
"""
import contextlib
import os

import torch
import torch.distributed as dist

from . import _lib as L
from . import heads, synth
from . import models as _models
from .models import CROP_POOL3, CROP_POOL4, opt_layers, up2_nhwc, up2_nhwc_bwd


def init_process_group(backend="nccl", device=None, **kw):
    """torch.distributed.init_process_group for the data-parallel step.  On the `nccl` backend (RCCL on ROCm) the collectives go
    to a HIGH-PRIORITY HIP stream (ProcessGroupNCCL.Options.is_high_priority_stream; SZN_RCCL_HIPRI=0 turns it off): the tile
    kernels of the backward pass hold 128-156 KiB of every CU's LDS and keep thousands of workgroups pending, and at normal
    priority RCCL's workgroups only got CUs when a compute kernel had drained -- measured with the one-rank communicator
    (profiles/r05_comm_hipri.json): fp32 wire +10.7 % per step at normal priority, +6.1 % at high priority; bf16 wire +10.9 % ->
    +2.4 %.  The reference is single-GPU (train.py:58,82-84) and has no counterpart."""
    if backend == "nccl" and os.environ.get("SZN_RCCL_HIPRI", "1") == "1":
        try:
            opts = dist.ProcessGroupNCCL.Options(is_high_priority_stream=True)
            return dist.init_process_group(backend, device_id=device, pg_options=opts, **kw)
        except (AttributeError, TypeError):
            pass
    if backend == "nccl":
        return dist.init_process_group(backend, device_id=device, **kw)
    return dist.init_process_group(backend, **kw)


def grad_report(names, stats, clip_state, factor):
    """host numbers of one step of TrainStep(clip=): stats = grad_stats ([n_seg][2] = {sum g, sum g*g} of the buffers as they stand),
    clip_state = {coef, norm, steps clipped, steps seen}, factor = what turns a buffer element into the true gradient (1 / (world x
    loss scale)).  -> dict(norm, coef, clipped, seen, sums={name: sum g}, norms={name: |g|})"""
    import math
    return dict(norm=float(clip_state[1]), coef=float(clip_state[0]), clipped=int(clip_state[2]), seen=int(clip_state[3]),
                sums={n: float(stats[i][0]) * factor for i, n in enumerate(names)},
                norms={n: math.sqrt(float(stats[i][1])) * factor if stats[i][1] >= 0 else float("nan") for i, n in enumerate(names)})


class GradBuckets(object):
    """Data-parallel exchange of the flat weight gradient: contiguous buckets in BACKWARD completion order.

    `layers` = [(name, offset, count)] in FORWARD order inside `flat`; backward finishes them last-to-first, so the
    tail of `flat` becomes final first.  A bucket is closed once it holds >= bucket_elems elements (or at the first
    layer) and its sum all-reduce is issued asynchronously (RCCL's own stream; gloo in the CPU tests) as soon as the
    bucket's earliest layer reports `layer_done`; `finish` waits for everything.  The 1/world scaling is applied by the
    optimizer kernel (grad_scale), not here.

    comm_dtype=torch.bfloat16 halves the bytes on the xGMI links (271 MB instead of 542 MB per step at E = 300).  Two forms:
      staged (direct=False)  the fp32 bucket is rounded into a 16-bit staging buffer, summed there and widened back into `flat`
                             by `finish` (two extra passes over the gradient; `.grad` stays fp32 and holds the sum);
      direct (direct=True)   the weight-gradient kernels write the 16-bit image themselves (szn_conv_desc_t.dw_lp) into
                             `self.stage`, the all-reduce sums it in place and the optimizer kernel reads it
                             (szn_adam_step_g16): no copy in, no copy out, `flat` is never touched.
    sharded=True: every bucket is reduce-scattered instead of all-reduced -- rank r then owns the summed slice
    `shard(bucket)` of it, runs the optimizer over that slice only (1/world of the pass) and `gather_weights` all-gathers the
    updated weight image (16-bit on the 16-bit paths: the same bytes on the links as a 16-bit all-reduce, 25 % fewer than an
    fp32 one).  enabled=False: no exchange at all (bench.py's comm-off timing at world > 1)."""

    def __init__(self, flat, layers, bucket_elems, extra=(), group=None, comm_dtype=torch.float32, force=None, enabled=True,
                 direct=False, sharded=False, tail=0):
        """force (default: SZN_FORCE_COMM=1): issue the bucket all-reduces even in a process group of ONE rank -- the whole
        exchange path (bucket slicing, RCCL's stream, the waits in front of the optimizer, the bf16 staging) then runs on a
        single GPU.  RCCL returns from an in-place sum over one rank without touching the device, so on the `nccl` backend the
        forced single-rank exchange uses the pre-multiplied sum (factor 1.0; AVG for 16-bit wire buffers): librccl's one-rank
        reduce kernel reads and writes every bucket on RCCL's stream while dgrad / wgrad keep running on the compute stream (same
        bits as no exchange).  tail: elements behind `flat` the staging buffer also needs (the fused head's padding rows)."""
        self.flat, self.extra, self.group = flat, list(extra), group
        ready = dist.is_available() and dist.is_initialized()
        self.world = dist.get_world_size(group) if ready else 1
        self.rank = dist.get_rank(group) if ready else 0
        if force is None:
            force = os.environ.get("SZN_FORCE_COMM", "0") == "1"
        self.active = bool(enabled) and ready and (self.world > 1 or bool(force))
        self.op = dist.ReduceOp.SUM
        if self.active and self.world == 1 and dist.get_backend(group) == "nccl":
            # one rank: sum == average == x * 1.0.  RCCL skips an in-place SUM entirely; the pre-multiplied sum (fp32 buckets) and
            # AVG (16-bit staging buffers: torch 2.10 hands RCCL a zero factor for a bf16 pre-multiplied sum) make it launch its
            # one-rank reduce kernel.
            which = "premul" if comm_dtype == torch.float32 else "avg"
            if which == "premul" and hasattr(dist, "_make_nccl_premul_sum"):
                self.op = dist._make_nccl_premul_sum(1.0)
            elif which == "avg":
                self.op = dist.ReduceOp.AVG
        self.buckets = []            # (start, end, name of the layer whose completion closes the bucket)
        end = None
        for name, off, cnt in reversed(layers):
            if end is None:
                end = off + cnt
            if end - off >= bucket_elems or name == layers[0][0]:
                self.buckets.append((off, end, name))
                end = None
        self.ready_after = {name: (o, e) for o, e, name in self.buckets}
        self.works = []
        self.issued = 0              # collective calls handed to the backend so far (tests / bench)
        self.comm_dtype = comm_dtype
        self.stage = None
        self.direct = bool(direct) and self.active and comm_dtype != torch.float32
        self.sharded = bool(sharded) and self.active
        if self.sharded and any((e - o) % (4 * self.world) for o, e, _ in self.buckets):
            raise L.SznError("sharded optimizer: every bucket must split into %d slices of whole 16-byte groups" % self.world)
        if self.active and comm_dtype != torch.float32:
            self.stage = torch.zeros(flat.numel() + tail, dtype=comm_dtype, device=flat.device)
        # self-diagnosis (bench.py): per step, when each bucket was handed to the backend and how long the compute stream then
        # stood still for it in finish() -- HIP events on the compute stream, read back by `timing_report`
        self.timing = False
        self._t0 = None
        self._tlog = []

    # ---- what the exchange works on ------------------------------------------------------------------
    def wire(self):
        """the buffer the collectives run on (the 16-bit staging buffer, or `flat` itself)"""
        return self.stage if self.stage is not None else self.flat

    def shard(self, o, e):
        """the slice [lo, hi) of bucket [o, e) whose sum this rank owns after a reduce-scatter"""
        n = (e - o) // self.world
        return o + self.rank * n, o + (self.rank + 1) * n

    def _emulate(self, t):
        """gloo has no reduce-scatter / all-gather-into-tensor for device memory (the one-GPU test harness runs CUDA tensors over
        gloo): an all-reduce of the whole bucket leaves the right sum in this rank's slice, a list all-gather moves the slices"""
        return t.is_cuda and dist.get_backend(self.group) == "gloo"

    def _collective(self, t, o, e):
        self.issued += 1
        if self.sharded and self.world > 1 and not self._emulate(t):
            lo, hi = self.shard(o, e)
            return dist.reduce_scatter_tensor(t[lo:hi], t[o:e], op=self.op, group=self.group, async_op=True)
        # (sharded, one rank: it owns everything -- the forced single-rank exchange keeps the all-reduce kernel)
        return dist.all_reduce(t[o:e], op=self.op, group=self.group, async_op=True)

    def begin_step(self):
        if self.timing and self.active:
            self._t0 = torch.cuda.Event(enable_timing=True)
            self._t0.record()
            self._cur = []

    def layer_done(self, name):
        if self.active and name in self.ready_after:
            o, e = self.ready_after[name]
            ev = None
            if self.timing and self._t0 is not None:
                ev = torch.cuda.Event(enable_timing=True)
                ev.record()
            if self.stage is None:
                self.works.append((self._collective(self.flat, o, e), None, name, ev))
            else:
                if not self.direct:
                    self.stage[o:e].copy_(self.flat[o:e])
                self.works.append((self._collective(self.stage, o, e), (o, e), name, ev))

    def finish(self):
        if self.active:
            for t in self.extra:
                self.issued += 1
                self.works.append((dist.all_reduce(t, op=self.op, group=self.group, async_op=True), None, "bias", None))
            for wk, span, name, ev in self.works:
                tm = self.timing and self._t0 is not None
                if tm:
                    e0 = torch.cuda.Event(enable_timing=True)
                    e0.record()
                wk.wait()
                if tm:
                    e1 = torch.cuda.Event(enable_timing=True)
                    e1.record()
                    self._cur.append((name, ev, e0, e1))
                if span is not None and not self.direct:
                    o, e = self.shard(*span) if (self.sharded and self.world > 1) else span
                    self.flat[o:e].copy_(self.stage[o:e])
            if self.timing and self._t0 is not None:
                self._tlog.append((self._t0, self._cur))
                self._t0 = None
        self.works = []

    def gather_weights(self, image, first_only=False, spans=False):
        """sharded optimizer: all-gather the slices of `image` (a tensor laid out like `flat`: the 16-bit weight image, or the
        fp32 masters) that the ranks just updated; returns the async works (wait before anything reads the gathered range: the next
        forward pass waits bucket by bucket, TrainStep.wait_weights).  first_only: the bucket of the first layers only (conv1_1 reads
        its fp32 master in the forward pass).  spans=True: [((start, end) of the bucket, work)] instead of the bare works."""
        works = []
        if self.sharded and self.world > 1:
            for o, e, _ in list(reversed(self.buckets))[:1 if first_only else None]:       # forward order: conv1_1's bucket first
                lo, hi = self.shard(o, e)
                self.issued += 1
                if self._emulate(image):
                    n = (e - o) // self.world
                    wk = dist.all_gather([image[o + r * n:o + (r + 1) * n] for r in range(self.world)], image[lo:hi].clone(),
                                         group=self.group, async_op=True)
                else:
                    wk = dist.all_gather_into_tensor(image[o:e], image[lo:hi], group=self.group, async_op=True)
                works.append(((o, e), wk) if spans else wk)
        return works

    def timing_report(self):
        """[{bucket, mib, issued_at_ms (since begin_step), wait_ms (compute stream stalled in finish)}] averaged over the logged
        steps + the exposed total; call after a device synchronize.  Clears the log."""
        log, self._tlog = self._tlog, []
        if not log:
            return None
        acc = {}
        order = []
        for t0, cur in log:
            for name, ev, e0, e1 in cur:
                a = acc.setdefault(name, [0.0, 0.0, 0])
                if name not in order:
                    order.append(name)
                a[0] += t0.elapsed_time(ev) if ev is not None else t0.elapsed_time(e0)
                a[1] += e0.elapsed_time(e1)
                a[2] += 1
        esz = 2 if self.stage is not None else 4
        size = {name: (e - o) * esz / 2.0 ** 20 for o, e, name in self.buckets}
        rows = [{"bucket": n, "mib": round(size.get(n, sum(t.numel() * 4 for t in self.extra) / 2.0 ** 20), 2),
                 "issued_at_ms": round(acc[n][0] / acc[n][2], 3), "wait_ms": round(acc[n][1] / acc[n][2], 3)} for n in order]
        return {"buckets": rows, "exposed_wait_ms": round(sum(r["wait_ms"] for r in rows), 3), "steps": len(log)}


def allreduce_param_grads(params, group=None):
    """mean of the per-rank gradients of an explicit parameter list (the autograd trainer paths: softmax / mse losses,
    seen-mask phase): one flat all-reduce.  No-op in a single process."""
    if not (dist.is_available() and dist.is_initialized()):
        return
    world = dist.get_world_size(group)
    if world == 1:
        return
    ps = [p for p in params if p.grad is not None]
    if not ps:
        return
    flat = torch.cat([p.grad.reshape(-1) for p in ps])
    dist.all_reduce(flat, group=group)
    flat /= world
    off = 0
    for p in ps:
        p.grad.copy_(flat[off:off + p.numel()].view_as(p.grad))
        off += p.numel()


class SeenmaskStep(object):
    """Phase 2 (BASELINE configs[2]) as one fused step: the body of trainer_seenmask.Trainer.train_epoch
    (trainer_seenmask.py:72-102) with the optimizer wiring of train.py:164-175, without autograd:

        backbone forward (train mode: Dropout2d on, like the reference's model.train(); no activation is kept -- the
        backbone is frozen)  ->  szn_seenmask_head: learned 64x64 stride-32 deconv + crop + 2-class cross entropy
        (size_average) + channel argmax + d(coarse) + d(seenmask_upscore.weight) straight from the 1/32 map, the
        (B,2,H,W) score never exists  ->  szn_seenmask_score_wgrad (seenmask_score weight / bias)  ->
        [one 98 KB all-reduce under data parallelism]  ->  Adam on the 24,578 head parameters.

    The three trainable tensors live in one flat fp32 buffer (the module's Parameters and .grads are views of it and of
    the flat gradient); the engine's fused head image (rows E, E+1 of [CP][4096]) and bias vector are rewritten in place
    after every update, so no weight image is rebuilt between steps.  Every kernel on this path reduces in a fixed order:
    two runs give bit-identical losses and weights."""

    def __init__(self, model, n_class, unseen, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, precision=None,
                 process_group=None):
        """n_class / unseen: the binary target of a pixel is "its label is one of the n_class classes and not in `unseen`"
        (trainer_seenmask.py:53-56); n_class = 0: step() is handed {0,1} targets already (other values are ignored)"""
        self.seen = heads.seen_set("SeenmaskStep", int(n_class), unseen)
        self.model, self.eng = model, model._engine
        if precision is not None:
            model.set_precision(precision)
        self.dev = model.conv1_1.weight.device
        if self.dev.type != "cuda":
            raise L.SznError("SeenmaskStep needs the model on the GPU")
        self.n_class = int(n_class)
        self.lr, self.betas, self.eps, self.wd = lr, betas, eps, weight_decay
        self.pg = process_group
        self.world = dist.get_world_size(process_group) if (dist.is_available() and dist.is_initialized()) else 1
        self.nstep = 0
        m = model
        F = m.fc7.out_channels
        self.F = F
        ps = (m.seenmask_score.weight, m.seenmask_upscore.weight, m.seenmask_score.bias)
        n = sum(p.numel() for p in ps)
        self.flat_p = torch.empty(n, device=self.dev)
        self.flat_g = torch.zeros(n, device=self.dev)
        self.m1, self.m2 = torch.zeros(n, device=self.dev), torch.zeros(n, device=self.dev)
        off = 0
        self.seg = {}
        for key, p in zip(("score_w", "up_w", "score_b"), ps):
            cnt = p.numel()
            if key == "score_w":             # (2,F,1,1): OHWI order == (2, F) rows
                src = p.detach().permute(0, 2, 3, 1).reshape(-1)
                view = lambda t, o=off, c=cnt: t[o:o + c].view(2, 1, 1, F).permute(0, 3, 1, 2)
            else:
                src = p.detach().reshape(-1)
                view = lambda t, o=off, c=cnt, sh=tuple(p.shape): t[o:o + c].view(sh)
            self.flat_p[off:off + cnt].copy_(src)
            p.data = view(self.flat_p)
            p.grad = view(self.flat_g)
            self.seg[key] = (off, cnt)
            off += cnt
        self.eng.mark_dirty()
        self.loss = torch.zeros(1, device=self.dev)
        self.stats = torch.zeros(2, device=self.dev)
        self.conf = torch.zeros(4, dtype=torch.int64, device=self.dev)     # [target][prediction] counts since the last reset
        self.head_ws = heads.Workspace(self.dev)
        self._ws2 = None

    def _head_images(self):
        """(rows E, E+1 of the fused head's weight image in the compute dtype, the same slice of its bias vector)"""
        m, img = self.model, self.eng._images
        E, CP, F = m.n_class, m.head_width, self.F
        return img["head.w"].view(CP, F)[E:E + 2], img["head.b"][E:E + 2]

    def step(self, x, target, dropout_masks=None):
        """x (B,3,H,W) f32 NCHW, target (B,H,W) int64 class labels (-1 = unlabelled), both on the GPU.
        -> (loss 0-dim device tensor, pred (B,H,W) int64 device tensor: 1 = "seen")"""
        m, eng = self.model, self.eng
        B, _, H, W = x.shape
        st = L.stream_ptr()
        ctx = eng.forward(x, train=m.training, masks=dropout_masks, keep=False)
        E, F = m.n_class, self.F
        M = B * ctx.h * ctx.w
        nb2 = L.load().szn_seenmask_score_wgrad_workspace_bytes(M, F)
        if self._ws2 is None or self._ws2.numel() < nb2 + M * 8:
            self._ws2 = torch.empty(nb2 + M * 8, dtype=torch.uint8, device=self.dev)
        dsc = self._ws2[nb2:nb2 + M * 8].view(torch.float32)
        pred = torch.empty(B, H, W, dtype=torch.int64, device=self.dev)
        (ow, nw), (ou, nu), (ob, nbias) = self.seg["score_w"], self.seg["up_w"], self.seg["score_b"]
        g = self.flat_g
        heads.seenmask(ctx.coarse, E, self.flat_p[ou:ou + nu], pred, target, self.n_class, self.seen, self.loss, self.stats, self.conf,
                       dsc, g[ou:ou + nu], ws=self.head_ws, stream=st)
        feat = ctx.relu7
        L.call("szn_seenmask_score_wgrad", L.dtype_code(feat.dtype), M, F, F, L.ptr(feat), L.ptr(dsc), L.ptr(g[ow:ow + nw]),
               L.ptr(g[ob:ob + nbias]), L.ptr(self._ws2), st)
        if self.world > 1:
            dist.all_reduce(g, group=self.pg)
        self._optimizer_step()
        return self.loss.reshape(()), pred

    def _optimizer_step(self):
        self.nstep += 1
        st = L.stream_ptr()
        gs = 1.0 / self.world
        rows, bias = self._head_images()
        (ow, nw) = self.seg["score_w"]
        n = self.flat_p.numel()
        lp16 = rows.dtype != torch.float32
        for o, cnt, lp in ((ow, nw, rows if lp16 else None), (ow + nw, n - ow - nw, None)):
            L.call("szn_adam_step", cnt, L.ptr(self.flat_p[o:o + cnt]), L.ptr(self.flat_g[o:o + cnt]), L.ptr(self.m1[o:o + cnt]),
                   L.ptr(self.m2[o:o + cnt]), float(self.lr), float(self.betas[0]), float(self.betas[1]), float(self.eps),
                   float(self.wd), self.nstep, gs, L.ptr(lp), L.dtype_code(lp.dtype) if lp is not None else 0, st)
        if not lp16:
            rows.copy_(self.flat_p[ow:ow + nw].view(2, self.F))
        ob, nbias = self.seg["score_b"]
        bias.copy_(self.flat_p[ob:ob + nbias])
        # seenmask_upscore.weight is read by the kernels in place (fp32 parameter storage): nothing to refresh

    def metrics(self, reset=True):
        """running train metrics (trainer_seenmask.py:87: label_accuracy_score on the binary maps with n_class classes)"""
        import numpy as np
        from .utils import _hist_to_metrics
        c = self.conf.cpu().numpy().reshape(2, 2)
        if reset:
            self.conf.zero_()
        h = np.zeros((max(self.n_class, 2), max(self.n_class, 2)))
        h[:2, :2] = c
        return _hist_to_metrics(h)

    def export_optimizer_state(self, optim):
        for key, p in (("score_w", self.model.seenmask_score.weight), ("score_b", self.model.seenmask_score.bias),
                       ("up_w", self.model.seenmask_upscore.weight)):
            o, cnt = self.seg[key]
            shape = lambda t: (t[o:o + cnt].view(2, 1, 1, self.F).permute(0, 3, 1, 2) if key == "score_w" else t[o:o + cnt].view(p.shape))
            stt = optim.state[p]
            stt['step'] = torch.tensor(float(self.nstep))
            stt['exp_avg'], stt['exp_avg_sq'] = shape(self.m1), shape(self.m2)


class TrainStep(object):
    def __init__(self, model, embeddings=None, optimizer="adam", lr=1e-5, momentum=0.99, weight_decay=0.0005,
                 precision=torch.bfloat16, fused_head=True, loss="cos", process_group=None, bucket_mb=25,
                 train_metrics=True, betas=(0.9, 0.999), eps=1e-8, bias_lr=None, bias_weight_decay=0.0,
                 adam_weight_decay=0.0, grad_comm_dtype=None, loss_scale=None, dynamic_loss_scale=None,
                 scale_growth=2.0, scale_backoff=0.5, scale_growth_interval=2000, force_comm=None, reserved_cus=None,
                 fused_adam=None, keep_grads=True, exchange=None, direct_wire=None, sharded=None, forced_unseen=None,
                 class_weight=None, size_average=False, sim_exclude=None, sim_temperature=None, pseudo=None, ohem=None,
                 rank_margin=None, rank_hardest=False, bias=None, ema=None, clip=None, accum=None):
        """Data-parallel knobs (the reference is single-GPU): grad_comm_dtype (SZN_GRAD_COMM = fp32 | bf16) = the
        wire format of the gradient buckets; exchange=False (SZN_GRAD_COMM=off) = no exchange at all (bench.py's comm-off timing);
        direct_wire (default: on for a 16-bit wire with keep_grads=False; SZN_WIRE_DIRECT=0 turns it off) = the weight-gradient
        kernels write the 16-bit wire image themselves and the optimizer kernel reads it (no staging copies; `.grad` of the
        weights is then None); sharded (SZN_SHARDED_OPT=1) = reduce-scatter + rank-sharded optimizer + all-gather of the weight
        image instead of all-reduce + replicated optimizer.
        forced_unseen (a list of class indices, trainer_fcn.py:110-112): the returned prediction is the forced-unseen one -- a pixel
        whose label is one of these classes is assigned among them, any other among the rest (szn_fused_head_grouped, group mode 2;
        the fused_head=False path: szn_embed_argmax_k mode 1 with the target).  Loss, gradients and updates do not change.
        loss="cross_entropy" (embeddings=None; the softmax FCN of train.py -c 1, utils.py:19-48 with trainer_fcn.py:133's
        size_average=False): K = C = model.n_class classes, the head is szn_fused_ce_head (fused_head=False: upscore -> szn_ce2d_fwd
        -> szn_ce2d_bwd -> head_backward), the prediction is the channel argmax; class_weight = optional [C] class weights.  Under
        data parallelism the update uses the mean of the rank gradients, as allreduce_param_grads gives the autograd route.
        loss="sim_ce" (utils.sim_ce_loss; szn_fused_simce_head): a softmax over the cosines of the classes outside sim_exclude (a list
        of class indices, the trainer's unseen classes; None: all compete) divided by sim_temperature (None: heads.SIM_TEMPERATURE),
        cross entropy against the label.  Fused head only: fused_head=False raises (no materialised kernels were built for it).
        loss="rank" (utils.rank_loss; szn_fused_rank_head): the hinge ranking loss -- the label's cosine must exceed the cosine of every
        other class outside sim_exclude (the same exclude set as sim_ce's) by rank_margin (None: heads.RANK_MARGIN); rank_hardest
        keeps the hardest negative alone instead of the sum of hinges.  Fused head only, like sim_ce; wherever the step treats
        sim_ce's exclude set specially (pseudo labels, ohem) it treats this one the same.
        pseudo=dict(unseen=[...], gamma=0.0, keep=0.3, conf_floor=-2.0) (embedding losses only): self-training on the pixels a
        hide_unseen dataset hides (label datasets.HIDDEN_LABEL).  After the forward pass szn_pseudo_head runs on the step's own head map
        (the 1/32 map, FCN8s: the 1/8 fused map) and stream: the calibrated rule at gamma picks the hidden pixels it gives to an unseen
        class with a similarity of at least conf_floor, per class the most confident `keep` of them take that class as their label, and
        the head -- fused or the fused_head=False referee -- trains on the relabelled target.  The train-metric histogram keeps the
        caller's target.  set_pseudo_active(False) makes the step the plain step again, launch for launch; with loss "sim_ce" or "rank" the active
        step empties sim_exclude (the unseen classes now have positives), the inactive one restores it.  pseudo_counts, a device (K,2) int64
        tensor, accumulates {candidates, selected} per class until the caller zeroes it; with keep_ctx the relabelled target of the last
        step stays in last_pseudo_target.  Under data parallelism the thresholds are those of each rank's own batch: nothing is
        exchanged, a rank's labels depend on its own pixels only.
        ohem=dict(keep=, thresh=None) (embedding losses only): hard-pixel mining.  After the forward pass (and after the pseudo-label pass,
        on its result: pseudo-labelled pixels are mined like real labels) szn_ohem_head runs on the step's own head map and stream: per
        image the `keep` (a share in (0, 1]) of the labelled pixels whose cosine to their own class embedding is lowest, and every pixel
        whose cosine lies below `thresh` (None: no threshold; bins of 1/512), keep their label, the others read heads.OHEM_DROP_LABEL,
        and the head -- fused or the fused_head=False referee -- trains on that target.  Hardness is the own-class cosine for all three
        losses; with loss "sim_ce" or "rank" the labels in the exclude set the step is using at that moment are neither counted nor dropped.  The
        caller's target tensor is never written and the train-metric histogram keeps it (with forced_unseen the dropped pixels of the
        train prediction compete in the seen group, like every ignored pixel).  set_ohem_active(False) makes the step the plain step
        again, launch for launch.  ohem_counts, a device (2,) int64 tensor, accumulates {evaluated, kept} over images and steps until the
        caller zeroes it; with keep_ctx the mined target of the last step stays in last_ohem_target.  Under data parallelism the cuts
        belong to each rank's own images: nothing is exchanged.
        bias=dict(unseen=[...], weight=lambda, hidden=datasets.HIDDEN_LABEL) (loss "sim_ce" only; utils.sim_ce_bias_loss;
        szn_fused_simce_bias_head): QFSL's unseen-bias term.  A pixel the dataset hides (label `hidden`) adds weight * -log of the
        probability mass its softmax over ALL classes puts on `unseen`; labelled pixels keep sim_ce's term, and the image's mean runs over
        both kinds.  The head reads the target the pseudo-label and mining passes leave: pixels that pseudo labelling relabels get the
        supervised term and only the still-hidden ones the bias term; mining neither counts nor drops hidden pixels (it evaluates labels
        in [0, K) only and copies every other label through).  `unseen` stays as given when active pseudo labels empty sim_exclude.
        set_bias_active(False) makes the step the plain sim_ce step again, launch for launch.  Under data parallelism nothing is
        exchanged: the term is per pixel.
        ema=dict(decay=, every=1, warmup=True): averaged weights (Polyak averaging).  ema_w / ema_b are fp32 copies of the flat
        parameter buffers; after the last optimizer launch of every `every`-th step szn_ema_step moves them towards the parameters,
        avg = param + D (avg - param) with D = min(decay, (1 + s) / (10 + s)) ^ every, s = the optimizer steps applied before this one
        (warmup=False: D = decay ^ every).  The launches sit in front of szn_loss_scale_update, so a step the dynamic loss scale skips
        on the device skips the average too, without a host sync; such a step that falls on an `every` boundary is simply lost to the
        average (the next update comes `every` steps later).  The average never feeds back into training.  averaged_weights() puts it
        under the model for a block (validation, export), ema_state_dict() / load_ema_state_dict() move it in and out of checkpoints,
        reset_ema() restarts it from the current parameters (import_optimizer_state does: a resumed run without a stored average),
        ema_updates counts the launches (for logs).  Plain data parallelism needs nothing: every rank holds the same parameters after
        the all-reduce and therefore the same average.  Refused with a ValueError: the sharded optimizer (the fp32 masters of the
        other ranks' slices are stale there), decay outside [0, 1), every < 1, and every > 1 while a stream capture is in progress
        (the host decides which steps update).  None (default): nothing changes, launch for launch.
        clip=dict(max_norm=M), M > 0: clipping by the global gradient norm (torch.nn.utils.clip_grad_norm_'s rule) and a per-layer
        gradient log; M = float('inf') takes the statistics only.  After the exchange and in front of the first optimizer launch two
        szn_grad_stats launches (weights -- the 16-bit wire image on the direct wire --, then biases) write {sum g, sum g*g} per layer
        into grad_stats (device double [n_seg][2]; grad_segments names the rows: every "<layer>.weight" in flat order, then every
        "<layer>.bias"), szn_clip_coef turns them into clip_state (device float[4] = {coef, norm, steps clipped, steps seen}) and every
        optimizer launch goes through the *_clipped entries, which multiply their gradient scale by coef.  The norm is that of the
        unscaled gradient (the loss scale and 1/world are divided out) over exactly the elements the optimizer launches update.  On
        the dynamic loss-scale path szn_clip_coef raises found_inf itself (a non-finite element makes the sum of squares non-finite)
        and the two szn_grad_check_finite launches are not issued; a skipped step moves neither counter.  grad_norms() reads the
        numbers back (a host sync).  The norm needs every gradient before any update, so the fc6 Adam epilogue and the early
        side-stream optimizer pass are off -- the path a data-parallel step takes anyway.  Data parallelism needs nothing: every rank
        reads the same all-reduced buffers.  Refused with a ValueError: a bad max_norm, and the sharded optimizer (a rank holds
        slices of the summed gradient only).  None (default): nothing changes, launch for launch.
        accum=dict(steps=A, average=True): gradient accumulation, A forward/backward passes per optimizer step.  step() is one
        micro-step: forward, head, loss, prediction, histogram, pseudo labels, mining and the bias term are per call and it returns the
        micro-batch's (loss, pred).  Behind everything that writes the flat gradient buffers two szn_grad_accum launches (weights, then
        biases) keep the window's running sum in acc_w / acc_b (fp32, as large as flat_gw / flat_gb): SET on the first call of a
        window, ADD on the ones in between -- and nothing else runs on those calls: no exchange (buckets.issued does not move), no
        overflow check, no statistics, no optimizer, no average, no loss-scale update; nstep stays and the weights are not marked
        dirty.  The A-th call (the boundary) runs FINAL, which leaves ((g1 + g2) + g3) + ... + gA -- torch's order for A backward()
        calls without zero_grad() -- in the flat gradient buffers themselves, then the whole exchange (begin_step, every bucket in
        buckets.buckets order, finish: not overlapped with backward, the other A - 1 micro-steps have none) and the unchanged
        optimizer step.  average=True multiplies the gradient scale by 1/A (the update, clip= and the gradient log see the mean of the
        micro-batch gradients), average=False uses the sum.  `.grad` of the parameters holds the micro-batch's gradient after a
        non-boundary call and the window's unscaled sum after a boundary call.  accum_steps = A, accum_pending = micro-steps summed
        since the last optimizer step (0 .. A - 1), last_applied = whether the last step() issued the optimizer launches (not whether
        the dynamic loss scale then skipped them on the device: applied_steps says that).  Every gradient is final only at the
        boundary, so -- as under clip= -- the fc6 Adam epilogue and the early side-stream optimizer pass are off, and so is the direct
        16-bit wire (the weight-gradient kernels would write the image of ONE micro-batch; the staged wire is used).  Dynamic loss
        scale: S changes only in szn_loss_scale_update, hence only at boundaries, so every micro-gradient of a window carries the same
        S; an inf / NaN in any of them survives the sum, the boundary's check raises found_inf, the optimizer entries and the average
        skip on the device and S backs off: the WHOLE window is lost.  ema= moves once per optimizer step.  reset_accum() restarts
        the window (the next call is a SET); import_optimizer_state calls it: pending micro-gradients are not checkpointed.  steps=1
        is None in every respect.  Refused with a ValueError: a bad dict, the sharded optimizer, and step() while a stream capture is
        in progress (the host decides which calls update).  None (default): nothing changes, launch for launch."""
        self._accum = None if accum is None else self._check_accum(accum)
        if self._accum is not None and self._accum[0] == 1:
            self._accum = None
        self.accum_steps = 1 if self._accum is None else self._accum[0]
        self._accum_scale = 1.0 / self.accum_steps if (self._accum is not None and self._accum[1]) else 1.0
        self.accum_pending = 0
        self.last_applied = False
        self.acc_w = self.acc_b = None
        self._clip = None if clip is None else self._check_clip(clip)
        self.grad_segments = self.grad_stats = self.clip_state = self.clip_scale = None
        self._ema = None if ema is None else self._check_ema(ema)
        self.ema_w = self.ema_b = None
        self.ema_updates = 0
        self._ema_in = False                                          # inside averaged_weights(): the buffers are exchanged
        if loss not in ("cos", "mse", "sim_ce", "rank", "cross_entropy"):
            raise L.SznError("TrainStep: loss must be 'cos', 'mse', 'sim_ce', 'rank' or 'cross_entropy', got %r" % (loss,))
        if (loss not in ("sim_ce", "rank") and sim_exclude is not None) or (loss != "sim_ce" and sim_temperature is not None):
            raise L.SznError("TrainStep: sim_exclude belongs to loss 'sim_ce' or 'rank' and sim_temperature to loss 'sim_ce', not %r"
                             % (loss,))
        if loss != "rank" and (rank_margin is not None or rank_hardest):
            raise L.SznError("TrainStep: rank_margin / rank_hardest belong to loss 'rank', not %r" % (loss,))
        if loss == "sim_ce" and not fused_head:
            raise L.SznError("TrainStep: the sim_ce loss runs on the fused head only; the materialised score goes through autograd "
                             "(utils.sim_ce_loss)")
        if loss == "rank" and not fused_head:
            raise L.SznError("TrainStep: the rank loss runs on the fused head only; the materialised score goes through autograd "
                             "(utils.rank_loss)")
        if bias is not None:
            if loss != "sim_ce":
                raise L.SznError("TrainStep: the bias loss belongs to loss 'sim_ce', not %r" % (loss,))
            if not isinstance(bias, dict) or embeddings is None:
                raise L.SznError("TrainStep: bias must be a dict(unseen=, weight=[, hidden=]) next to the class embeddings, got %r" % (bias,))
            heads.bias_args(loss, bias, len(embeddings))              # host checks only: nothing has touched a device yet
        if pseudo is not None:
            pseudo = self._check_pseudo(pseudo, loss)
        if ohem is not None:
            ohem = self._check_ohem(ohem, loss)
        self.ce = loss == "cross_entropy"
        if self.ce and (embeddings is not None or forced_unseen is not None):
            raise L.SznError("TrainStep: the cross-entropy head takes no embeddings and no forced_unseen classes")
        if not self.ce and embeddings is None:
            raise L.SznError("TrainStep: the %s loss needs the class embeddings" % loss)
        self.model = model
        self.eng = model._engine
        # FCN8s (models.FCN8s: public skip head, not in the reference): two more Conv2d layers in the flat buffers and the head
        # chain upscore2 -> +score_pool4 -> upscore_pool4 -> +score_pool3 -> fused head over 8x8 cells, run without autograd
        self.layers = opt_layers(model)
        self.is8 = len(self.layers) > 17
        if self.is8 and not fused_head:
            raise L.SznError("TrainStep(FCN8s) runs the fused stride-8 head only; the materialised score goes through autograd")
        model.set_precision(precision)
        self.dev = model.conv1_1.weight.device
        if self.dev.type != "cuda":
            raise L.SznError("TrainStep needs the model on the GPU")
        self.head_ws = heads.Workspace(self.dev)        # the fused head's scratch and prepared embedding tables, kept across steps
        if self.ce:
            self.emb = None
            self.K = self.E = model.n_class
            if self.K > L.MAX_CLASSES:
                raise L.SznError("TrainStep: the cross-entropy head holds at most %d classes, got %d" % (L.MAX_CLASSES, self.K))
            self.class_weight = None
            if class_weight is not None:
                self.class_weight = torch.as_tensor(class_weight).to(self.dev, torch.float32).contiguous()
                if self.class_weight.numel() != self.K:
                    raise L.SznError("TrainStep: class_weight has %d entries for %d classes" % (self.class_weight.numel(), self.K))
            self.size_average = bool(size_average)
        else:
            self.emb = heads.embeddings(embeddings, model.n_class, self.dev, fused=fused_head)
            self.K, self.E = self.emb.shape
        self.opt, self.lr, self.momentum, self.wd = optimizer, lr, momentum, weight_decay
        # the reference wiring (train.py:126-133): biases at 2 x lr without weight decay; Adam has no weight decay at all
        self.betas, self.eps = betas, eps
        self.adam_wd = adam_weight_decay
        self.bias_lr = 2 * lr if bias_lr is None else bias_lr
        self.bias_wd = bias_weight_decay
        env_comm = os.environ.get("SZN_GRAD_COMM", "fp32")
        if grad_comm_dtype is None:
            grad_comm_dtype = torch.bfloat16 if env_comm == "bf16" else torch.float32
        self.grad_comm_dtype = grad_comm_dtype
        self.exchange = (env_comm != "off") if exchange is None else bool(exchange)
        self.keep_grads = bool(keep_grads)
        if direct_wire is None:
            direct_wire = os.environ.get("SZN_WIRE_DIRECT", "1") == "1" and not self.keep_grads
        self._want_direct = bool(direct_wire) and grad_comm_dtype != torch.float32
        self._want_sharded = (os.environ.get("SZN_SHARDED_OPT", "0") == "1") if sharded is None else bool(sharded)
        self.fused_head, self.loss_kind = fused_head, loss
        self.forced_unseen = None if forced_unseen is None else [int(k) for k in forced_unseen]
        if self.forced_unseen is not None and any(not 0 <= k < self.K for k in self.forced_unseen):
            raise L.SznError("TrainStep: forced_unseen names a class outside [0, %d)" % self.K)
        self._unseen_cs = L.class_set(self.forced_unseen) if self.forced_unseen is not None else None
        self._group = 0 if self.forced_unseen is None else 2          # heads.embed group mode: plain / forced unseen
        self._sim_kw = {}                                             # heads.embed's extra keywords of loss "sim_ce" / "rank"
        if loss == "sim_ce":
            excl = sorted(set(int(k) for k in (sim_exclude or [])))
            if any(not 0 <= k < self.K for k in excl) or len(excl) >= self.K:
                raise L.SznError("TrainStep: sim_exclude must name classes of [0, %d) and leave one competing" % self.K)
            temp = float(heads.SIM_TEMPERATURE if sim_temperature is None else sim_temperature)
            if not 0 < temp < float("inf"):
                raise L.SznError("TrainStep: sim_temperature must be positive and finite, got %r" % (sim_temperature,))
            self._sim_kw = dict(exclude=excl, temperature=temp)
        if loss == "rank":
            excl = sorted(set(int(k) for k in (sim_exclude or [])))
            if any(not 0 <= k < self.K for k in excl) or self.K - len(excl) < 2:
                raise L.SznError("TrainStep: sim_exclude must name classes of [0, %d) and leave two competing for loss 'rank'" % self.K)
            margin = float(heads.RANK_MARGIN if rank_margin is None else rank_margin)
            if not 0 <= margin < float("inf"):
                raise L.SznError("TrainStep: rank_margin must be finite and >= 0, got %r" % (rank_margin,))
            self._sim_kw = dict(exclude=excl, margin=margin, hardest=bool(rank_hardest))
        self._bias = None if bias is None else dict(bias)             # heads.embed's bias keyword, see set_bias_active
        self._bias_active = False
        self.set_bias_active(bias is not None)
        self._pseudo = None                                           # szn_pseudo_head's arguments, see set_pseudo_active
        self._pseudo_active = False
        self.last_pseudo_target = None                                # (keep_ctx) the relabelled target the last step's head read
        if pseudo is not None:
            self._init_pseudo(pseudo)
        self._ohem = None                                             # szn_ohem_head's arguments, see set_ohem_active
        self._ohem_active = False
        self.last_ohem_target = None                                  # (keep_ctx) the mined target the last step's head read
        if ohem is not None:
            self._init_ohem(ohem)
        # static loss scaling for the fp16 path: gradients below 6e-8 vanish in IEEE half, so d(loss)/d(coarse) is multiplied
        # by loss_scale in fp32 before it enters the 16-bit backward pass and the optimizer kernel divides it out again
        # (grad_scale).  The .grad views then hold loss_scale x gradient.  bf16 / fp32 need none.
        # The cross-entropy head's loss is a SUM over pixels (trainer_fcn.py:133): each coarse position of d(coarse) collects the
        # gradients (|d| <= 1 per class) of the up to (2 S)^2 pixels its taps reach -- ~1e3 at stride 32, 2^18 x B times the
        # 1/(B N)-scaled cosine gradient.  4096 x that overflows IEEE half (65504) at the head already, so the CE step starts at
        # scale 1 (its gradients are far above fp16's subnormal range) and may back off below 1 (floor 2^-8) if a batch overflows.
        # The MSE head's gradient is 2 (s - e) x the same geometric factor S^2 / (B N_b): linear in the residual and not bounded by
        # 1 / |s| as the cosine's is.  A trained net's residual is below 1 (cosine-sized gradients); a freshly initialised head
        # emits scores of order 1e3.  The worst case for overflow is a SMALL batch of small images, where S^2 / (B N_b) is largest:
        # at B N_b / S^2 = 18 (two 96 x 96 images) 512 is the largest power of two that keeps the scaled head gradient under 65504
        # for per-channel residuals up to 2^10.  At the product shape (eight 512 x 512 images) the factor is ~450 x smaller, 512 is
        # merely conservative there and the dynamic scale grows (x2 per 2000 clean steps); too high a start costs skipped steps
        # at once, too low a start only resolution that growth wins back.
        # The sim_ce head starts at the cosine head's 4096.  Its per-pixel gradient is (1/T) sum_k (p_k - y_k) d cos_k / d s with
        # |d cos_k / d s| <= 1 / |s| (the cosine head's own bound) and sum_k |p_k - y_k| <= 2, so |dL/ds| <= 2 / (T |s|): the cosine
        # bound times 2 / T, 20 x at the default T = 0.1, with the same 1 / (B N_b) and the same geometry.  The bound is reached only
        # by a pixel whose whole probability sits on wrong classes that all pull one way; a position's S^2 weights / (B N_b) times
        # 4096 x 2 / (T |s|) stays under 65504 once |s| > 0.07 at the worst shape above (B N_b / S^2 = 18), and the scores of a fresh
        # or trained head are orders above that.  Should a batch overflow all the same, the dynamic scale pays log2(2 / T) ~ 5
        # skipped steps at the very start (x 1/2 per overflowing step) and nothing afterwards.
        # The rank head starts there too: |dL/ds| <= 2 V / |s| for a pixel with V violated hinges (V <= 1 with rank_hardest), the
        # cosine bound times 2 V.  A fresh head violates most of its up to K - 2 hinges, so the sum form may exceed sim_ce's 2 / T
        # at first; the dynamic scale pays for that with a few halvings at the start and grows back as the hinges clear.
        # The bias term of sim_ce keeps sim_ce's start: a hidden pixel's gradient is (weight / T) sum_k (p_k - q_k) d cos_k / d s with
        # sum_k |p_k - q_k| <= 2 (two distributions), so |dL/ds| <= 2 weight / (T |s|), sim_ce's bound times weight.
        fp16_scale0 = 1.0 if self.ce else (512.0 if loss == "mse" else 4096.0)
        self._loss_scale0 = float(loss_scale) if loss_scale is not None else (fp16_scale0 if precision == torch.float16 else 1.0)
        # dynamic loss scaling (default for fp16): the scale, the overflow flag and the count of APPLIED optimizer steps live
        # on the device (include/szn.h, szn_grad_check_finite / szn_*_step_scaled / szn_loss_scale_update); a step whose
        # gradients contain inf / NaN leaves masters, moments and weight images untouched and halves the scale -- no host
        # synchronisation, identical decisions on every data-parallel rank (the flag is read from the all-reduced gradient)
        self.dynamic = (precision == torch.float16) if dynamic_loss_scale is None else bool(dynamic_loss_scale)
        self.scale_cfg = (float(scale_growth), float(scale_backoff), int(scale_growth_interval), 2.0 ** -8 if self.ce else 1.0,
                          2.0 ** 32)
        self.scale_state = None
        self._scaled = self.dynamic or self._loss_scale0 != 1.0
        self.pg = process_group
        self.world = dist.get_world_size(process_group) if (dist.is_available() and dist.is_initialized()) else 1
        if self.ce and self.size_average and self.world > 1:
            # the mean over the valid pixels of the whole data-parallel batch would need the pixel count all-reduced first
            raise L.SznError("TrainStep: size_average=True cross entropy is single-process only")
        self.force_comm = force_comm
        self.train_metrics = train_metrics
        self.nstep = 0
        self._flatten()
        self._buckets(bucket_mb)
        if self._ema is not None:
            if self.buckets.sharded:
                raise ValueError("TrainStep: ema= does not run with the sharded optimizer, whose fp32 masters of the other ranks' slices are stale")
            self.reset_ema()
        if self._clip is not None:
            if self.buckets.sharded:
                raise ValueError("TrainStep: clip= does not run with the sharded optimizer, where a rank holds slices of the summed gradient only")
            self._init_clip()
        if self._accum is not None:
            if self.buckets.sharded:
                raise ValueError("TrainStep: accum= does not run with the sharded optimizer, which reduce-scatters every step's gradient")
            self.acc_w, self.acc_b = torch.empty_like(self.flat_gw), torch.empty_like(self.flat_gb)
        # CUs the persistent one-block-per-CU backward kernels (conv3x3_regw dgrad, conv_wgrad_taps) leave to RCCL's workgroups
        # while an exchange is in flight (default SZN_RESERVED_CUS, 0 = none; only when buckets are actually exchanged)
        if reserved_cus is None:
            reserved_cus = int(os.environ.get("SZN_RESERVED_CUS", "0"))
        self.eng.reserved_cus = int(reserved_cus) if self.buckets.active else 0
        if self.dynamic:
            self.scale_state = torch.tensor([self._loss_scale0, 0.0, 0.0, 0.0], device=self.dev)
        self.hist = torch.zeros(3, self.K, self.K, dtype=torch.int64, device=self.dev)
        self.loss = torch.zeros(1, device=self.dev)
        self.stats = None
        # fused stride-32 head: d(loss)/d(coarse), reused across steps of one shape and dtype (_dcoarse_buffer)
        self._dcoarse = self._dcoarse_key = None
        # the head layers' report to the gradient buckets, last-to-first: the flat order ends (..., score_pool3, score_pool4, score_fr)
        self._head_layers = ("score_fr", "score_pool4", "score_pool3") if self.is8 else ("score_fr",)
        # Adam for fc6 / fc7 (89 % of the weights) applied in the epilogue of their weight-gradient kernels (szn_conv2d_wgrad_adam):
        # only where a gradient is final when its kernel ends -- one rank (no exchange), no dynamic loss scale -- and on the 16-bit
        # paths (the kernel with that epilogue is a 16-bit MFMA kernel).  SZN_FUSED_ADAM=0 / fused_adam=False: the separate pass.
        # keep_grads=False: the fused layers' gradients are not written to the flat gradient buffer at all (nothing reads them in
        # a training loop that calls zero_grad() next, train.py:170-175); the default keeps .grad meaningful.
        if fused_adam is None:
            fused_adam = os.environ.get("SZN_FUSED_ADAM", "1") == "1"
        self._own_stream = None          # see step(): the non-blocking stream of a small step
        # clip= / accum=: every gradient must be final before any update, so no update may ride in a weight-gradient kernel
        self.fused_adam = bool(fused_adam and optimizer == "adam" and not self.dynamic and not self.buckets.active
                               and self.flat_w_lp is not None and os.environ.get("SZN_EARLY_ADAM", "auto") != "1"
                               and self._clip is None and self._accum is None)
        if self.fused_adam and not self.keep_grads:
            # the fused layers' gradients are consumed inside their weight-gradient kernel and never stored: `.grad` must not
            # look like a gradient (the reference keeps .grad valid until zero_grad(); keep_grads=True restores that)
            for n in os.environ.get("SZN_FUSED_ADAM_LAYERS", "fc6").split(","):
                if n in self.woff and n in ("fc6", "fc7"):
                    getattr(model, n).weight.grad = None
        self._pending_gather = []    # sharded optimizer: [((start, end), work)] all-gathers of the weight image nobody has waited for yet
        self.gather_wait_log = []    # (tests) (layer that asked, bucket start, bucket end) in the order the waits were issued
        self.keep_ctx = False        # tests: keep the forward state of the last step (activations stay alive one step longer)
        self.last_ctx = None
        self.last_fuse3 = None           # (FCN8s, keep_ctx) the 1/8 fused map of the last step

    def set_bias_active(self, active):
        """turn the unseen-bias term of a step built with bias= on or off; off, the step is the plain sim_ce step launch for launch"""
        if self._bias is None:
            if active:
                raise L.SznError("TrainStep: set_bias_active(True) on a step built without bias=")
            return
        self._bias_active = bool(active)
        if self._bias_active:
            self._sim_kw["bias"] = self._bias
        else:
            self._sim_kw.pop("bias", None)

    # ---- self-training pseudo labels ----------------------------------------------------------------------------------------
    @staticmethod
    def _check_pseudo(cfg, loss):
        """pseudo= checked as far as the host alone can (before anything touches a device) -> (unseen, gamma, permille, conf_floor)"""
        import math
        if loss == "cross_entropy":
            raise L.SznError("TrainStep: pseudo labels need an embedding loss ('cos' | 'mse' | 'sim_ce' | 'rank'): the cross-entropy head has "
                             "no unseen-class scores")
        if not isinstance(cfg, dict):
            raise L.SznError("TrainStep: pseudo must be a dict(unseen=, gamma=, keep=, conf_floor=), got %r" % (cfg,))
        cfg = dict(cfg)
        unseen = sorted(set(int(k) for k in (cfg.pop("unseen", None) or [])))
        gamma, keep, floor = cfg.pop("gamma", 0.0), cfg.pop("keep", 0.3), cfg.pop("conf_floor", -2.0)
        if cfg:
            raise L.SznError("TrainStep: pseudo takes unseen, gamma, keep and conf_floor, not %s" % sorted(cfg))
        if not unseen or unseen[0] < 0:
            raise L.SznError("TrainStep: pseudo['unseen'] must name the unseen classes (got %r)" % (unseen,))
        gamma, floor = float(0.0 if gamma is None else gamma), float(floor)
        if not (math.isfinite(gamma) and math.isfinite(floor)):
            raise L.SznError("TrainStep: pseudo gamma and conf_floor must be finite (got %r, %r)" % (gamma, floor))
        return unseen, gamma, heads.pseudo_permille(keep), floor

    def _init_pseudo(self, checked):
        unseen, gamma, permille, floor = checked
        if unseen[-1] >= self.K or len(unseen) >= self.K:
            raise L.SznError("TrainStep: pseudo['unseen'] must name some, not all, classes of [0, %d)" % self.K)
        self._pseudo = dict(unseen=L.class_set(unseen), gamma=gamma, permille=permille, floor=floor)
        self.pseudo_counts = torch.zeros(self.K, 2, dtype=torch.int64, device=self.dev)
        self._pseudo_step_counts = torch.zeros(self.K, 2, dtype=torch.int64, device=self.dev)
        self._pseudo_ws = None
        self._sim_exclude = self._sim_kw.get("exclude")
        self.set_pseudo_active(True)

    def set_pseudo_active(self, active):
        """turn the pseudo-label pass of a step built with pseudo= on or off; off, the step is the plain step launch for launch"""
        if self._pseudo is None:
            if active:
                raise L.SznError("TrainStep: set_pseudo_active(True) on a step built without pseudo=")
            return
        self._pseudo_active = bool(active)
        if self.loss_kind in ("sim_ce", "rank"):
            self._sim_kw["exclude"] = [] if self._pseudo_active else self._sim_exclude

    def _head_target(self, stride, fmap, target, H, W, st):
        """the caller's target through the pseudo-label pass, then the mining pass (each the identity while it is inactive)"""
        return self._ohem_target(stride, fmap, self._pseudo_target(stride, fmap, target, H, W, st), H, W, st)

    def _pseudo_target(self, stride, fmap, target, H, W, st):
        """the target the head trains on: the caller's, or -- pseudo labels active -- szn_pseudo_head's relabelled copy of it"""
        if not self._pseudo_active:
            return target
        p = self._pseudo
        nbytes = heads.pseudo_workspace_bytes(stride, fmap, self.emb, H, W)
        if self._pseudo_ws is None or self._pseudo_ws.numel() < nbytes:
            self._pseudo_ws = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        out = torch.empty_like(target)
        heads.pseudo_call(stride, fmap, self.emb, H, W, target, p["unseen"], p["gamma"], p["permille"], p["floor"], heads.HIDDEN_LABEL,
                          out, self._pseudo_ws, st, counts=self._pseudo_step_counts)
        self.pseudo_counts += self._pseudo_step_counts
        self.last_pseudo_target = out if self.keep_ctx else None
        return out

    # ---- hard-pixel mining --------------------------------------------------------------------------------------------------
    @staticmethod
    def _check_ohem(cfg, loss):
        """ohem= checked as far as the host alone can (before anything touches a device) -> (permille, thresh; -2.0: no threshold)"""
        import math
        if loss == "cross_entropy":
            raise L.SznError("TrainStep: ohem needs an embedding loss ('cos' | 'mse' | 'sim_ce' | 'rank'): hardness is the cosine to the "
                             "pixel's own class embedding, which the cross-entropy head does not have")
        if not isinstance(cfg, dict):
            raise L.SznError("TrainStep: ohem must be a dict(keep=, thresh=None), got %r" % (cfg,))
        cfg = dict(cfg)
        if "keep" not in cfg:
            raise L.SznError("TrainStep: ohem needs keep, the share of every image's labelled pixels to train on, in (0, 1]")
        keep, thresh = cfg.pop("keep"), cfg.pop("thresh", None)
        if cfg:
            raise L.SznError("TrainStep: ohem takes keep and thresh, not %s" % sorted(cfg))
        try:
            thresh = -2.0 if thresh is None else float(thresh)
        except (TypeError, ValueError):
            raise L.SznError("TrainStep: ohem thresh must be a finite number or None (got %r)" % (thresh,))
        if not math.isfinite(thresh):
            raise L.SznError("TrainStep: ohem thresh must be finite or None (got %r)" % (thresh,))
        return heads.ohem_permille(keep), thresh

    def _init_ohem(self, checked):
        permille, thresh = checked
        self._ohem = dict(permille=permille, thresh=thresh)
        self.ohem_counts = torch.zeros(2, dtype=torch.int64, device=self.dev)
        self._ohem_step_counts = None                                 # (B,2), sized by the first batch
        self._ohem_ws = None
        self._ohem_skip = (None, None)                                # (the exclude list, its class set)
        self.set_ohem_active(True)

    def set_ohem_active(self, active):
        """turn the mining pass of a step built with ohem= on or off; off, the step is the plain step launch for launch"""
        if self._ohem is None:
            if active:
                raise L.SznError("TrainStep: set_ohem_active(True) on a step built without ohem=")
            return
        self._ohem_active = bool(active)

    def _ohem_target(self, stride, fmap, target, H, W, st):
        """the target the head trains on: the one handed in, or -- mining active -- szn_ohem_head's copy of it with the easy pixels dropped"""
        if not self._ohem_active:
            return target
        o = self._ohem
        B = target.shape[0]
        nbytes = heads.ohem_workspace_bytes(stride, fmap, self.emb, H, W)
        if self._ohem_ws is None or self._ohem_ws.numel() < nbytes:
            self._ohem_ws = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        if self._ohem_step_counts is None or self._ohem_step_counts.shape[0] != B:
            self._ohem_step_counts = torch.zeros(B, 2, dtype=torch.int64, device=self.dev)
        excl = self._sim_kw.get("exclude") if self.loss_kind in ("sim_ce", "rank") else None      # the set the head uses in this very step
        if excl is not self._ohem_skip[0]:
            self._ohem_skip = (excl, L.class_set(excl))
        out = torch.empty_like(target)
        heads.ohem_call(stride, fmap, self.emb, H, W, target, self._ohem_skip[1], o["permille"], o["thresh"], heads.OHEM_DROP_LABEL, out,
                        self._ohem_ws, st, counts=self._ohem_step_counts)
        self.ohem_counts += self._ohem_step_counts.sum(0)
        self.last_ohem_target = out if self.keep_ctx else None
        return out

    # the class-embedding matrix: assigning a new tensor (or calling invalidate_head_prep() after writing into it behind torch's back --
    # a raw kernel does not bump _version, and a new tensor may reuse the address of the old one) makes the fused head rebuild its tables
    @property
    def emb(self):
        return self._emb

    @emb.setter
    def emb(self, t):
        self._emb = t
        self.invalidate_head_prep()

    def invalidate_head_prep(self):
        self.head_ws.invalidate()

    @property
    def loss_scale(self):
        """the factor the .grad views currently carry (dynamic scaling: read back from the device -- a host sync; tests only)"""
        return float(self.scale_state[0].item()) if self.dynamic else self._loss_scale0

    def _scale(self, t, dtype):
        """t (fp32 d loss / d head input) x loss scale in fp32, as `dtype`"""
        return (t.float() * (self.scale_state[0] if self.dynamic else self._loss_scale0)).to(dtype)

    @property
    def applied_steps(self):
        """optimizer steps that were actually applied (dynamic loss scaling skips overflowed ones)"""
        return int(self.scale_state[2].item()) if self.dynamic else self.nstep

    # ---- flat parameter / gradient / moment storage ----------------------------------------------------
    def _flatten(self):
        m = self.model
        ws = [getattr(m, n).weight for n in self.layers]
        bs = [getattr(m, n).bias for n in self.layers]
        nw, nb = sum(p.numel() for p in ws), sum(p.numel() for p in bs)
        CP, E, F = m.head_width, m.n_class, m.fc7.out_channels
        self.flat_w = torch.empty(nw, device=self.dev)
        # score_fr is the last layer of the flat layout: the (CP - E) rows behind its bias slot complete the fused head's
        # bias vector (seenmask_score + zero padding), so the engine can use one contiguous view of it
        self._flat_b_store = torch.zeros(nb + CP - E, device=self.dev)
        self.flat_b = self._flat_b_store[:nb]
        # gradients: the fused head's wgrad (CP rows: score_fr | seenmask_score | padding) writes straight into score_fr's
        # slot at the END of the flat buffers; the (CP - E) rows behind it land in a tail that nothing reads
        self._flat_gw_store = torch.zeros(nw + (CP - E) * F, device=self.dev)
        self._flat_gb_store = torch.zeros(nb + CP - E, device=self.dev)
        self.flat_gw = self._flat_gw_store[:nw]
        self.flat_gb = self._flat_gb_store[:nb]
        self.woff, self.boff = {}, {}
        off = 0
        for n, p in zip(self.layers, ws):
            co, ci, kh, kw = p.shape
            seg = self.flat_w[off:off + p.numel()].view(co, kh, kw, ci)
            seg.copy_(p.detach().permute(0, 2, 3, 1))
            p.data = seg.permute(0, 3, 1, 2)                       # channels_last view of the flat master
            p.grad = self.flat_gw[off:off + p.numel()].view(co, kh, kw, ci).permute(0, 3, 1, 2)
            self.woff[n] = (off, p.numel())
            off += p.numel()
        off = 0
        for n, p in zip(self.layers, bs):
            seg = self.flat_b[off:off + p.numel()]
            seg.copy_(p.detach())
            p.data = seg
            p.grad = self.flat_gb[off:off + p.numel()]
            self.boff[n] = (off, p.numel())
            off += p.numel()
        self.state = {}
        for key, flat in (("w", self.flat_w), ("b", self.flat_b)):
            if self.opt == "adam":
                self.state[key] = (torch.zeros_like(flat), torch.zeros_like(flat))
            else:
                self.state[key] = (torch.zeros_like(flat),)
        # low-precision weight image written by the optimizer kernel itself (no separate cast pass per step)
        self.flat_w_lp = None
        self.eng.lp_views = {}
        if self.eng.dtype in (torch.bfloat16, torch.float16):
            # (CP - E) x F extra elements behind score_fr's slot: the fused head's weight image [CP][F] is then a view
            store = torch.zeros(nw + (CP - E) * F, device=self.dev, dtype=self.eng.dtype)
            store[:nw].copy_(self.flat_w)
            self._flat_w_lp_store = store
            self.flat_w_lp = store[:nw]
            for n in self.layers[:-1]:
                co, ci, kh, kw = getattr(m, n).weight.shape
                o, cnt = self.woff[n]
                if n.startswith("score_pool"):
                    continue                                  # padded images are assembled per step (_skip_images)
                self.eng.lp_views[n] = self.flat_w_lp[o:o + cnt].view(co, kh, kw, ci)
            assert self.layers[-1] == "score_fr"
            o, cnt = self.woff["score_fr"]
            bo, bc = self.boff["score_fr"]
            assert o + cnt == nw and bo + bc == nb
            self.eng.lp_views["head"] = (store[o:o + CP * F].view(CP, F), self._flat_b_store[bo:bo + CP])
            self.eng._seen_versions = None
        self.eng.mark_dirty()
        # per-layer gradient targets handed to the engine (OHWI views of the flat gradient)
        self.grads = {}
        self.skip = {}               # FCN8s: per skip layer (padded weight image, dgrad image, bias image, gradient scratch)
        for n in self.layers[:-1]:
            if n.startswith("score_pool"):
                ci = getattr(m, n).in_channels
                dt = self.eng.dtype
                self.skip[n] = dict(w=torch.zeros(CP, 1, 1, ci, device=self.dev, dtype=dt),
                                    wT=torch.zeros(ci, 1, 1, CP, device=self.dev, dtype=dt),
                                    b=torch.zeros(CP, device=self.dev), gw=torch.empty(CP, 1, 1, ci, device=self.dev),
                                    gb=torch.empty(CP, device=self.dev))
                continue
            p = getattr(m, n).weight
            co, ci, kh, kw = p.shape
            o, cnt = self.woff[n]
            bo, bc = self.boff[n]
            self.grads[n] = (self.flat_gw[o:o + cnt].view(co, kh, kw, ci), self.flat_gb[bo:bo + bc])
        o, cnt = self.woff["score_fr"]
        bo, bc = self.boff["score_fr"]
        assert o + cnt == nw and bo + bc == nb       # score_fr is the last layer of both flat layouts
        self.head_gw = self._flat_gw_store[o:o + CP * F].view(CP, 1, 1, F)
        self.head_gb = self._flat_gb_store[bo:bo + CP]
        self.grads["head"] = (self.head_gw, self.head_gb)
        self.grads["_flat_bias"] = self._flat_gb_store      # lets the engine zero all bias gradients with one fill

    def _buckets(self, bucket_mb):
        layers = [(n,) + self.woff[n] for n in self.layers]
        m = self.model
        CP, E, F = m.head_width, m.n_class, m.fc7.out_channels
        # direct 16-bit wire: bf16 compute path only (the kernels that write the image are the 16-bit weight-gradient kernels; the
        # dynamic loss scale's overflow check reads fp32 gradients; the FCN8s skip layers copy theirs in from scratch buffers;
        # under accum= the image would be that of one micro-batch)
        direct = self._want_direct and not self.dynamic and not self.is8 and self.eng.dtype != torch.float32 and self._accum is None
        # sharded optimizer: not with the dynamic loss scale either -- after a reduce-scatter a rank holds summed gradients for its own slices
        # only, so the overflow check (szn_grad_check_finite over the whole buffer) would see different data on different ranks and the ranks
        # would disagree on skipping the step / backing the scale off
        self.buckets = GradBuckets(self.flat_gw, layers, bucket_mb * (1 << 20) // 4, extra=[self.flat_gb], group=self.pg,
                                   comm_dtype=self.grad_comm_dtype, force=self.force_comm, enabled=self.exchange, direct=direct,
                                   sharded=self._want_sharded and not self.dynamic, tail=(CP - E) * F)
        self._gather = []
        if self.buckets.direct:
            stage = self.buckets.stage
            lp = {}
            for n in self.layers[:-1]:
                o, cnt = self.woff[n]
                lp[n] = stage[o:o + cnt]
                getattr(m, n).weight.grad = None         # never written on this path (the wire image is the gradient)
            o, cnt = self.woff["score_fr"]
            lp["head"] = stage[o:o + CP * F]
            m.score_fr.weight.grad = None
            self.grads["_lp"] = lp

    # ---- one training step -----------------------------------------------------------------------------
    def step(self, x, target):
        """x (B,3,H,W) f32 NCHW, target (B,H,W) int64 (-1 ignore), both on the GPU.
        Returns (loss 0-dim device tensor, pred (B,H,W) int64 device tensor).  Under accum= this is one micro-step."""
        if self._accum is not None and torch.cuda.is_current_stream_capturing():
            raise ValueError("TrainStep: accum= cannot be captured into a graph, the host decides which calls update the weights")
        work = self._small_step_stream(x)
        if work is None:
            return self._step(x, target)
        # A small step (the reference's one image per step, train.py:82-84) whose fc6 update rides in its weight-gradient kernel: that
        # kernel goes to a stream confined to part of the CUs (models._Engine._masked_stream).  Such a stream is a BLOCKING one -- it
        # synchronises with the null stream launch by launch (measured: 2.57 -> 3.5 ms) -- so when the caller is on the null stream the
        # whole step moves to a non-blocking stream of its own, forked from and joined to the caller's.
        cur = torch.cuda.current_stream(self.dev)
        work.wait_stream(cur)
        with torch.cuda.stream(work):
            out = self._step(x, target)
        cur.wait_stream(work)
        for t in out:
            t.record_stream(cur)
        return out

    def _small_step_stream(self, x):
        if not self.fused_adam or self.eng.dtype == torch.float32 or torch.cuda.is_current_stream_capturing():
            return None
        if not _models.masked_stream_wanted(x.shape[0] * x.shape[2] * x.shape[3]):
            return None
        if torch.cuda.current_stream(self.dev) != torch.cuda.default_stream(self.dev):
            return None                  # already on a non-blocking stream of the caller's
        if self._own_stream is None:
            self._own_stream = torch.cuda.Stream(device=self.dev)
        return self._own_stream

    def _step(self, x, target):
        """forward -> the head map (the 1/32 map, or FCN8s' 1/8 fused map) -> head (fused, or the materialised referee) -> loss
        scale -> backward -> exchange -> optimizer -> confusion histogram (accum=: backward -> szn_grad_accum, and on the window's last
        call -> exchange -> optimizer)"""
        m, eng = self.model, self.eng
        if self._ema_in:
            raise L.SznError("TrainStep: no training step inside averaged_weights(): the model holds the averaged weights")
        B, _, H, W = x.shape
        st = L.stream_ptr()
        eng.keep_prepool = bool(self.keep_ctx)          # tests that read the forward state need the un-pooled tensors too
        ctx = eng.forward(x, train=m.training)
        self.last_ctx = ctx if self.keep_ctx else None
        pred = torch.empty(B, H, W, dtype=torch.int64, device=self.dev)
        stats = torch.empty(B, 2, device=self.dev)
        skips = None
        if self.is8:
            fuse4, fuse3 = self._chain8(ctx)
            dmap = torch.zeros(B, fuse3.shape[1], fuse3.shape[2], m.head_width, device=self.dev, dtype=torch.float32)
            self._head(8, fuse3, self._head_target(8, fuse3, target, H, W, st), H, W, stats, pred, dmap, st)
            if self._scaled:                            # d(fuse3) is scaled in fp32; the chain's backward converts
                dmap = self._scale(dmap, torch.float32)
            dcoarse, skips = self._chain8_backward(ctx, fuse4, dmap)
        else:
            head_target = self._head_target(32, ctx.coarse, target, H, W, st)
            if self.fused_head:
                dcoarse = self._dcoarse_buffer(ctx)
                self._head(32, ctx.coarse, head_target, H, W, stats, pred, dcoarse, st)
            else:
                dcoarse = self._referee(ctx, head_target, stats, pred, st)
            if self._scaled:
                dcoarse = self._scale(dcoarse, eng.dtype)
        self.stats = stats
        acc = self._accum is not None
        boundary = not acc or self.accum_pending == self.accum_steps - 1
        done = (lambda name: None) if acc else self._layer_done_hook(B * H * W)
        self._fused_begin()
        try:
            if not acc:
                self.buckets.begin_step()
            # rows [0,E) of the fused head gradient ARE score_fr's slot of the flat gradient (seenmask_score is frozen in phase 1):
            # nothing to copy, the first bucket can go as soon as the head wgrad has been queued
            eng.backward(ctx, dcoarse, self.grads, backbone=True, layer_done=done,
                         head_first=lambda: [done(n) for n in self._head_layers], skips=skips)
            # FCN8s: the skip layers' bias gradients live in the flat bias buffer the engine zeroes first: re-apply them
            for n, s in self.skip.items():
                bo, bc = self.boff[n]
                self.flat_gb[bo:bo + bc].copy_(s["gb"][:self.E])
            if acc:
                self._accum_launch(boundary, st)
            else:
                self.buckets.finish()
            if boundary:
                self._optimizer_step()
            self.last_applied = boundary
        finally:                         # an error in between must not leave the engine armed with this step's Adam arguments
            eng.fused_opt, eng.fused_done = None, set()
        if self.train_metrics:
            L.call("szn_confusion_hist_k", target.numel(), self.K, L.ptr(target), L.ptr(pred), None, L.ptr(self.hist), st)
        return self.loss.reshape(()), pred

    # ---- the head: fused (heads.py) or materialised --------------------------------------------------------------------------
    def _head(self, stride, fmap, target, H, W, stats, pred, dmap, st):
        """the fused head on the NHWC map `fmap`: loss, stats, pred, d(fmap) into the zero-padded `dmap`"""
        if self.ce:
            heads.ce(stride, fmap, self.K, H, W, pred, target, self.class_weight, self.size_average, self.loss, stats, dmap,
                     ws=self.head_ws, stream=st)
        else:
            heads.embed(self.loss_kind, stride, fmap, self.emb, H, W, pred, target, self.loss, stats, dmap, self._group,
                        self._unseen_cs, ws=self.head_ws, stream=st, **self._sim_kw)

    def _dcoarse_buffer(self, ctx):
        """d(loss)/d(coarse) of the fused head: it writes channels [0, E) and the padding channels stay zero, so the buffer of the
        previous step is reused without a fill (everything that read it was queued on this stream -- or joined -- before this step)"""
        key = (ctx.B, ctx.h, ctx.w, self.model.head_width, torch.float32 if self._scaled else self.eng.dtype)
        if self._dcoarse_key != key:
            self._dcoarse, self._dcoarse_key = torch.zeros(key[:4], device=self.dev, dtype=key[4]), key
        return self._dcoarse

    def _referee(self, ctx, target, stats, pred, st):
        """fused_head=False (stride 32): the materialised head as the in-step referee -- upscore -> loss forward and prediction ->
        loss backward -> head_backward; cosine / mse with szn_embed_argmax_k, cross entropy with szn_ce2d_*.  -> fp32 d(coarse)"""
        eng = self.eng
        B, H, W, K = ctx.B, ctx.H, ctx.W, self.K
        f = eng.upscore(ctx)
        ws = torch.empty(L.load().szn_loss_workspace_bytes(B, H, W), dtype=torch.uint8, device=self.dev)
        df = torch.empty_like(f)
        if self.ce:                      # szn_ce2d_fwd writes the channel-argmax prediction too
            cw, sa = L.ptr(self.class_weight), int(self.size_average)
            L.call("szn_ce2d_fwd", B, K, H, W, L.ptr(f), L.ptr(target), cw, sa, L.ptr(self.loss), L.ptr(stats), L.ptr(pred),
                   L.ptr(ws), st)
            L.call("szn_ce2d_bwd", B, K, H, W, L.ptr(f), L.ptr(target), cw, sa, L.ptr(stats), None, L.ptr(df), st)
        else:
            E, emb = self.E, L.ptr(self.emb)
            kind = "cosine" if self.loss_kind == "cos" else "mse"
            L.call("szn_%s_loss_fwd" % kind, B, E, H, W, K, L.ptr(f), L.ptr(target), emb, None, L.ptr(self.loss), L.ptr(stats),
                   L.ptr(ws), st)
            grouped = self.forced_unseen is not None          # forced unseen: mode 1, the group from the target
            L.call("szn_embed_argmax_k", B, E, H, W, K, L.ptr(f), emb, int(grouped), self._unseen_cs, None,
                   L.ptr(target) if grouped else None, L.ptr(pred), st)
            L.call("szn_%s_loss_bwd" % kind, B, E, H, W, K, L.ptr(f), L.ptr(target), emb, None, L.ptr(stats), None, L.ptr(df), st)
        return eng.head_backward(ctx, df=df)[0]

    # ---- FCN8s head chain (forward and backward by hand: no autograd objects on the step path) ----------------------------
    def _skip_images(self):
        """padded [CP][Ci] images of score_pool3 / score_pool4 (rows >= E stay zero) + their dgrad transposes, from the flat
        masters the optimizer kernel just wrote"""
        E = self.E
        code = L.dtype_code(self.eng.dtype)
        for n, s in self.skip.items():
            o, cnt = self.woff[n]
            ci = s["w"].shape[3]
            src = self.flat_w_lp if (self.flat_w_lp is not None) else self.flat_w
            s["w"][:E].copy_(src[o:o + cnt].view(E, 1, 1, ci))
            bo, bc = self.boff[n]
            s["b"][:E].copy_(self.flat_b[bo:bo + bc])
            L.call("szn_pack_weight_dgrad", code, s["w"].shape[0], 1, 1, ci, L.ptr(s["w"]), L.ptr(s["wT"]), L.stream_ptr())

    def _chain8(self, ctx):
        """upscore2(score_fr) + score_pool4c -> upscore_pool4 -> + score_pool3c: -> (fuse4, fuse3), fp32 NHWC at 1/16 and 1/8"""
        eng = self.eng
        self._skip_images()
        s3, s4 = self.skip["score_pool3"], self.skip["score_pool4"]
        up2 = up2_nhwc(ctx.coarse)
        sp4 = eng._conv(ctx.pools[3][1], None, 0, relu=False, out_f32=True, w=s4["w"], b=s4["b"])
        n4, m4 = up2.shape[1:3]
        fuse4 = up2 + sp4[:, CROP_POOL4:CROP_POOL4 + n4, CROP_POOL4:CROP_POOL4 + m4]
        up4 = up2_nhwc(fuse4)
        sp3 = eng._conv(ctx.pools[2][1], None, 0, relu=False, out_f32=True, w=s3["w"], b=s3["b"])
        n3, m3 = up4.shape[1:3]
        fuse3 = (up4 + sp3[:, CROP_POOL3:CROP_POOL3 + n3, CROP_POOL3:CROP_POOL3 + m3]).contiguous()
        self.last_fuse3 = fuse3 if self.keep_ctx else None      # tests: the 1/8 map the head read
        return fuse4, fuse3

    def _chain8_backward(self, ctx, fuse4, dfuse3):
        """backward of the skip chain from the (scaled) fp32 d(fuse3): the skip layers' weight / bias gradients, their input
        gradients (which join the backbone chain at the pool3 / pool4 outputs) -> (d(coarse) in the compute dtype, skips)"""
        eng, CP, E = self.eng, self.model.head_width, self.E
        dt = eng.dtype
        skips = {}
        dmap = dfuse3
        for (name, pool, crop, pi, up_shape) in (("score_pool3", ctx.pools[2][1], CROP_POOL3, 2, fuse4.shape),
                                                 ("score_pool4", ctx.pools[3][1], CROP_POOL4, 3, ctx.coarse.shape)):
            s = self.skip[name]
            Bp, hp, wp, ci = pool.shape
            nn, mm = dmap.shape[1:3]
            dsp = torch.zeros(Bp, hp, wp, CP, device=self.dev, dtype=dt)
            dsp[:, crop:crop + nn, crop:crop + mm] = dmap
            o, cnt = self.woff[name]
            # the copy into the flat gradient runs as the wgrad's `after` hook: on the weight-gradient stream when
            # SZN_WGRAD_STREAM=1 moves these launches off the main stream (a copy queued on the main stream would race them)
            eng._wgrad(pool, dsp, s["gw"], s["gb"], ci, CP, 1, 0,
                       after=lambda o=o, cnt=cnt, s=s, ci=ci: self.flat_gw[o:o + cnt].view(E, 1, 1, ci).copy_(s["gw"][:E]))
            skips[pi] = eng._dgrad(dsp, None, pool.shape, 0, wT=s["wT"])
            dmap = up2_nhwc_bwd(dmap, tuple(up_shape))
        eng._join_wgrad()
        return (dmap if dmap.dtype == dt else dmap.to(dt)), skips

    # ---- optimizer --------------------------------------------------------------------------------------
    def _layer_done_hook(self, pixels):
        """layer_done callback of one backward pass.  Small steps (the reference's batch size of one image: train.py:82-84) leave most
        of the chip idle during conv5_3 .. conv1_1's backward kernels (32 .. 124 tiles on 256 CUs) while the HBM-bound optimizer pass
        over fc6 / fc7 / score_fr -- 90 % of the parameters, final as soon as fc6's dgrad has been queued -- waits for the end of the
        step: on one rank without dynamic loss scaling that slice is updated on a second stream from layer_done("conv5_3") on (fc6's
        dgrad, the last reader of fc6's weight image, is queued before it).  Same kernels, same values.  At B = 8 the MFMA-bound backward
        kernels slow down by what the overlapped pass takes (profiles/r03_ablations.txt section 17), and at B = 1 the 16-bit step does not gain
        either (3.09 -> 3.12 ms: the pass takes CUs from the few-tile kernels it was meant to hide behind), but the fp32 step does (15.41
        -> 14.90 ms, profiles/r04_ablations.txt section 7): SZN_EARLY_ADAM = 0 / 1 forces it off / on, default = fp32 steps of at most
        2 x 512 x 512 pixels."""
        self._early = False
        base = self.buckets.layer_done
        mode = os.environ.get("SZN_EARLY_ADAM", "auto")
        on = mode == "1" or (mode == "auto" and pixels <= 2 * 512 * 512 and self.eng.dtype == torch.float32)
        if not on or self.buckets.active or self.dynamic or self.is8 or "fc6" not in self.woff:
            return base
        if self._clip is not None:       # the early pass would update fc6 .. score_fr before the step's norm is known
            return base

        def done(name):
            base(name)
            if name == "conv5_3":
                if getattr(self, "_side", None) is None:
                    self._side = torch.cuda.Stream(device=self.dev)
                cur = torch.cuda.current_stream()
                self._side.wait_stream(cur)
                with torch.cuda.stream(self._side):
                    self._opt_launch("w", self.woff["fc6"][0], self.flat_w.numel(), self.nstep + 1)
                self._early = True
        return done

    def _fused_begin(self):
        """hand the engine the Adam arguments of the layers whose update rides in their weight-gradient kernel (this step = nstep + 1)"""
        eng = self.eng
        eng.fused_done = set()
        eng.fused_opt = None
        if not self.fused_adam:
            return
        m1, m2 = self.state["w"]
        gs = 1.0 / (self.world * self._loss_scale0)
        out = {}
        # fc6 only by default: its 1,568 tiles run 6 rounds, so update traffic and K loops of different CUs overlap (852 us against
        # 447 + 523 separately at B = 8); fc7's 256 tiles are one round -- K loop, then everybody's update: 155 us against 70 + 75
        for n in os.environ.get("SZN_FUSED_ADAM_LAYERS", "fc6").split(","):
            if n not in self.woff or n not in ("fc6", "fc7"):
                continue
            o, cnt = self.woff[n]
            a = L.AdamArgs()
            a.param, a.exp_avg, a.exp_avg_sq = self.flat_w[o:o + cnt].data_ptr(), m1[o:o + cnt].data_ptr(), m2[o:o + cnt].data_ptr()
            a.w_lp, a.w_lp_dtype = self.flat_w_lp[o:o + cnt].data_ptr(), L.dtype_code(self.flat_w_lp.dtype)
            a.lr, a.beta1, a.beta2, a.eps = float(self.lr), float(self.betas[0]), float(self.betas[1]), float(self.eps)
            a.weight_decay, a.step, a.grad_scale = float(self.adam_wd), self.nstep + 1, gs
            out[n] = (a, self.keep_grads)
        eng.fused_opt = out

    def _opt_launch(self, key, lo, hi, nstep):
        """one optimizer launch over elements [lo, hi) of the flat weight ("w") or bias ("b") buffers, on the current stream"""
        if hi <= lo:
            return
        st = L.stream_ptr()
        dyn = self.scale_state
        gs = self.grad_factor()
        flat, grad = (self.flat_w, self.flat_gw) if key == "w" else (self.flat_b, self.flat_gb)
        g16 = key == "w" and self.buckets.direct      # the summed 16-bit wire image IS the gradient (szn_*_step_g16)
        if g16:
            grad = self.buckets.stage
        lr, wd = (self.lr, self.wd) if key == "w" else (self.bias_lr, self.bias_wd)
        lp_on = key == "w" and self.flat_w_lp is not None
        lp_code = L.dtype_code(self.flat_w_lp.dtype) if self.flat_w_lp is not None else 0
        lp = L.ptr(self.flat_w_lp[lo:hi]) if lp_on else None
        n = hi - lo
        if self._clip is not None:       # the *_clipped entries: supersets of the three forms below, gradient scale x clip_state[0]
            gcode = L.dtype_code(grad.dtype)
            if self.opt == "adam":
                m1, m2 = self.state[key]
                awd = float(self.bias_wd if key == "b" else self.adam_wd)
                L.call("szn_adam_step_clipped", n, L.ptr(flat[lo:hi]), L.ptr(grad[lo:hi]), gcode, L.ptr(m1[lo:hi]), L.ptr(m2[lo:hi]),
                       float(lr), float(self.betas[0]), float(self.betas[1]), float(self.eps), awd, nstep, gs, L.ptr(dyn),
                       L.ptr(self.clip_state), lp, lp_code, st)
            else:
                (buf,) = self.state[key]
                L.call("szn_sgd_momentum_step_clipped", n, L.ptr(flat[lo:hi]), L.ptr(grad[lo:hi]), gcode, L.ptr(buf[lo:hi]), float(lr),
                       float(self.momentum), float(wd), int(nstep == 1), gs, L.ptr(dyn), L.ptr(self.clip_state), lp, lp_code, st)
            return
        if self.opt == "adam":           # train.py:130-133 (Adam has no weight decay in the reference wiring)
            m1, m2 = self.state[key]
            awd = float(self.bias_wd if key == "b" else self.adam_wd)
            if g16:
                L.call("szn_adam_step_g16", n, L.ptr(flat[lo:hi]), L.ptr(grad[lo:hi]), L.dtype_code(grad.dtype), L.ptr(m1[lo:hi]),
                       L.ptr(m2[lo:hi]), float(lr), float(self.betas[0]), float(self.betas[1]), float(self.eps), awd, nstep, gs, lp,
                       lp_code, st)
            elif self.dynamic:
                L.call("szn_adam_step_scaled", n, L.ptr(flat[lo:hi]), L.ptr(grad[lo:hi]), L.ptr(m1[lo:hi]), L.ptr(m2[lo:hi]), float(lr),
                       float(self.betas[0]), float(self.betas[1]), float(self.eps), awd, L.ptr(dyn), gs, lp, lp_code, st)
            else:
                L.call("szn_adam_step", n, L.ptr(flat[lo:hi]), L.ptr(grad[lo:hi]), L.ptr(m1[lo:hi]), L.ptr(m2[lo:hi]), float(lr),
                       float(self.betas[0]), float(self.betas[1]), float(self.eps), awd, nstep, gs, lp, lp_code, st)
        else:                            # train.py:126-129
            (buf,) = self.state[key]
            if g16:
                L.call("szn_sgd_momentum_step_g16", n, L.ptr(flat[lo:hi]), L.ptr(grad[lo:hi]), L.dtype_code(grad.dtype), L.ptr(buf[lo:hi]),
                       float(lr), float(self.momentum), float(wd), int(nstep == 1), gs, lp, lp_code, st)
            elif self.dynamic:
                L.call("szn_sgd_momentum_step_scaled", n, L.ptr(flat[lo:hi]), L.ptr(grad[lo:hi]), L.ptr(buf[lo:hi]), float(lr),
                       float(self.momentum), float(wd), L.ptr(dyn), gs, lp, lp_code, st)
            else:
                L.call("szn_sgd_momentum_step", n, L.ptr(flat[lo:hi]), L.ptr(grad[lo:hi]), L.ptr(buf[lo:hi]), float(lr),
                       float(self.momentum), float(wd), int(nstep == 1), gs, lp, lp_code, st)

    def _optimizer_step(self):
        self.nstep += 1
        st = L.stream_ptr()
        dyn = self.scale_state
        if self._clip is not None:       # statistics of the (already all-reduced) gradients, the step's coefficient, the overflow flag
            self._clip_launch(st)
        elif self.dynamic:               # raise the overflow flag from the (already all-reduced) gradients
            L.call("szn_grad_check_finite", self.flat_gw.numel(), L.ptr(self.flat_gw), L.ptr(dyn), st)
            L.call("szn_grad_check_finite", self.flat_gb.numel(), L.ptr(self.flat_gb), L.ptr(dyn), st)
        whi = self.flat_w.numel()
        if getattr(self, "_early", False):           # fc6 .. score_fr were updated under the backward pass (_layer_done_hook)
            torch.cuda.current_stream().wait_stream(self._side)
            whi = self.woff["fc6"][0]
            self._early = False
        if self.buckets.sharded:
            # reduce-scattered buckets: this rank holds the sum of one slice per bucket and updates only that (1/world of the pass);
            # the updated slices of the weight image are all-gathered (16-bit on the 16-bit paths; the fp32 masters of the other
            # ranks' slices go stale here -- gather_masters() before anything reads them: checkpoints)
            for o, e, _ in self.buckets.buckets:
                lo, hi = self.buckets.shard(o, e)
                self._opt_launch("w", lo, hi, self.nstep)
            image = self.flat_w_lp if self.flat_w_lp is not None else self.flat_w
            works = self.buckets.gather_weights(image, spans=True)
            if self.flat_w_lp is not None:       # conv1_1's kernel reads the fp32 master (3 input channels: no 16-bit image): its bucket's too
                works += self.buckets.gather_weights(self.flat_w, first_only=True, spans=True)
            # Nobody waits here: the all-gathers (forward order, conv1_1's 2 MiB bucket first, fc6's 196 MB fourth) run on RCCL's stream
            # under the tail of this step and the head of the next forward pass, whose layers wait for THEIR bucket only
            # (_Engine.weight_gate -> wait_weights(layer)): conv1_1 .. conv5_3 of the next step run while fc6's image is still on the links
            self._pending_gather = works
            self.eng.weight_gate = self.wait_weights if works else None       # (one rank owns every slice: nothing to wait for)
            # masters (16-bit paths) and moments (every path) of the other ranks' slices are stale from here on
            self._masters_stale = self.buckets.world > 1
        else:
            # the weight ranges not already updated inside their weight-gradient kernels (_fused_begin)
            lo = 0
            for n in sorted(self.eng.fused_done, key=lambda n: self.woff[n][0]):
                o, cnt = self.woff[n]
                if o < whi:
                    self._opt_launch("w", lo, min(o, whi), self.nstep)
                    lo = o + cnt
            self._opt_launch("w", lo, whi, self.nstep)
        self.eng.fused_opt = None
        self.eng.fused_done = set()
        self._opt_launch("b", 0, self.flat_b.numel(), self.nstep)
        if self._ema is not None:        # after the step's last optimizer launch, before the found_inf flag is cleared
            self._ema_launch(st)
        if self.dynamic:
            g, b, iv, lo, hi = self.scale_cfg
            L.call("szn_loss_scale_update", L.ptr(dyn), g, b, iv, lo, hi, st)
        self.eng.mark_dirty()

    def wait_weights(self, layer=None):
        """sharded optimizer: make the current stream wait for the pending all-gathers of the weight image -- of the bucket that holds
        `layer` (and of every bucket in front of it: forward order), or of all of them (None).  Called by the engine in front of every
        layer's first use of its weights in the next forward pass, and by everything else that reads parameters (gather_masters)."""
        pend = getattr(self, "_pending_gather", None)
        if not pend:
            return
        if layer is None:
            upto = self.flat_w.numel()
        else:
            o, cnt = self.woff["score_fr" if layer == "head" else layer]
            upto = o + cnt
        keep = []
        for (o, e), wk in pend:
            if o < upto:
                wk.wait()                # (the compute stream waits, not the host)
                self.gather_wait_log.append((layer, o, e))
            else:
                keep.append(((o, e), wk))
        self._pending_gather = keep
        if not keep:
            self.eng.weight_gate = None

    def gather_masters(self):
        """sharded optimizer: bring the optimizer moments -- and on a 16-bit path the fp32 masters (the fp32 path all-gathers them as the
        weight image in every step) -- of the other ranks' slices up to date on this rank (all-gather over the bucket slices).  Call before
        reading model parameters / optimizer state: checkpoints, export."""
        self.wait_weights()
        if not getattr(self, "_masters_stale", False):
            return
        ts = ([self.flat_w] if self.flat_w_lp is not None else []) + list(self.state["w"])
        for t in ts:
            for wk in self.buckets.gather_weights(t):
                wk.wait()
        self._masters_stale = False

    # ---- checkpoint compatibility (reference dict keys: trainer_fcn.py:281-288) ------------------------------
    def _param_slots(self):
        m = self.model
        for n in self.layers:
            p = getattr(m, n).weight
            co, ci, kh, kw = p.shape
            o, cnt = self.woff[n]
            yield p, "w", lambda t, o=o, cnt=cnt, co=co, ci=ci, kh=kh, kw=kw: t[o:o + cnt].view(co, kh, kw, ci).permute(0, 3, 1, 2)
            b = getattr(m, n).bias
            bo, bc = self.boff[n]
            yield b, "b", lambda t, bo=bo, bc=bc: t[bo:bo + bc]

    def export_optimizer_state(self, optim):
        """expose the flat moments as per-parameter state of a torch-style optimizer object (views, no copies), so that
        `optim.state_dict()` written into a checkpoint has the layout torch.optim.Adam / SGD would have produced"""
        self.gather_masters()
        for p, key, view in self._param_slots():
            st = optim.state[p]
            if self.opt == "adam":
                st['step'] = torch.tensor(float(self.applied_steps))
                st['exp_avg'] = view(self.state[key][0])
                st['exp_avg_sq'] = view(self.state[key][1])
            else:
                st['momentum_buffer'] = view(self.state[key][0]) if self.applied_steps > 0 else None

    def import_optimizer_state(self, optim):
        """inverse of export_optimizer_state (resume: train.py:135-136 loads `optim_state_dict` into the optimizer)"""
        steps = []
        for p, key, view in self._param_slots():
            st = optim.state.get(p, {})
            if self.opt == "adam" and 'exp_avg' in st:
                view(self.state[key][0]).copy_(st['exp_avg'])
                view(self.state[key][1]).copy_(st['exp_avg_sq'])
                steps.append(int(st.get('step', 0)))
            elif self.opt != "adam" and st.get('momentum_buffer') is not None:
                view(self.state[key][0]).copy_(st['momentum_buffer'])
                steps.append(1)
        if steps:
            self.nstep = max(steps)
            if self.dynamic:
                self.scale_state[2] = float(self.nstep)
        if self._ema is not None:        # a resumed run: the average restarts from the loaded weights unless load_ema_state_dict follows
            self.reset_ema()
        self.reset_accum()               # ... and its window: pending micro-gradients are not checkpointed

    # ---- gradient accumulation (accum=) -------------------------------------------------------------------------------------
    @staticmethod
    def _check_accum(cfg):
        """accum= checked on the host (before anything touches a device) -> (steps, average)"""
        if not isinstance(cfg, dict) or "steps" not in cfg or not set(cfg) <= {"steps", "average"}:
            raise ValueError("TrainStep: accum must be a dict(steps=, average=True), got %r" % (cfg,))
        steps, average = cfg["steps"], cfg.get("average", True)
        if isinstance(steps, bool) or not isinstance(steps, int) or steps < 1:
            raise ValueError("TrainStep: accum steps must be an integer >= 1, got %r" % (steps,))
        if not isinstance(average, bool):
            raise ValueError("TrainStep: accum average must be True or False, got %r" % (average,))
        return steps, average

    def reset_accum(self):
        """forget the micro-gradients summed so far: the next step() opens a window (SZN_ACCUM_SET).  A no-op without accum=."""
        self.accum_pending = 0

    def _accum_launch(self, boundary, st):
        """behind everything that wrote the flat gradient buffers in this micro-step: the window's running sum (weights, then biases) and,
        on the window's last call, the whole exchange of the summed buffers"""
        mode = L.ACCUM_FINAL if boundary else (L.ACCUM_SET if self.accum_pending == 0 else L.ACCUM_ADD)
        for a, g in ((self.acc_w, self.flat_gw), (self.acc_b, self.flat_gb)):
            L.call("szn_grad_accum", g.numel(), L.ptr(a), L.ptr(g), mode, st)
        if not boundary:
            self.accum_pending += 1
            return
        self.accum_pending = 0
        if self.buckets.active:
            self.buckets.begin_step()
            for _, _, name in self.buckets.buckets:
                self.buckets.layer_done(name)
            self.buckets.finish()

    # ---- gradient statistics and gradient-norm clipping (clip=) -------------------------------------------------------------
    @staticmethod
    def _check_clip(cfg):
        """clip= checked on the host (before anything touches a device) -> max_norm"""
        if not isinstance(cfg, dict) or set(cfg) != {"max_norm"}:
            raise ValueError("TrainStep: clip must be a dict(max_norm=), got %r" % (cfg,))
        try:
            m = float(cfg["max_norm"])
        except (TypeError, ValueError):
            raise ValueError("TrainStep: clip max_norm must be a number, got %r" % (cfg["max_norm"],))
        if isinstance(cfg["max_norm"], bool) or not m > 0.0:
            raise ValueError("TrainStep: clip max_norm must be > 0 (float('inf'): statistics only), got %r" % (cfg["max_norm"],))
        return m

    def _init_clip(self):
        import ctypes
        if len(self.layers) > L.GRAD_STATS_MAX_SEGS:
            raise ValueError("TrainStep: clip= holds at most %d layers per buffer" % L.GRAD_STATS_MAX_SEGS)
        self.grad_segments = [n + ".weight" for n in self.layers] + [n + ".bias" for n in self.layers]
        nl = len(self.layers)
        self.grad_stats = torch.zeros(2 * nl, 2, dtype=torch.float64, device=self.dev)
        self.clip_state = torch.tensor([1.0, 0.0, 0.0, 0.0], device=self.dev)
        self.clip_scale = torch.ones(1, device=self.dev)      # dynamic path: the loss scale the last step's gradients carried
        self._seg_tabs = []
        for off in (self.woff, self.boff):                    # HOST tables szn_grad_stats reads during the call
            ends = [off[n][0] + off[n][1] for n in self.layers]
            self._seg_tabs.append((ctypes.c_int64 * nl)(*ends))
        nb = max(L.load().szn_grad_stats_workspace_bytes(t.numel(), nl) for t in (self.flat_gw, self.flat_gb))
        self._clip_ws = torch.empty(nb, dtype=torch.uint8, device=self.dev)

    def _clip_launch(self, st):
        nl = len(self.layers)
        gw = self.buckets.stage[:self.flat_gw.numel()] if self.buckets.direct else self.flat_gw     # (as _opt_launch reads it)
        for i, g in enumerate((gw, self.flat_gb)):
            L.call("szn_grad_stats", g.numel(), L.ptr(g), L.dtype_code(g.dtype), nl, self._seg_tabs[i], L.ptr(self.grad_stats[i * nl:]),
                   L.ptr(self._clip_ws), st)
        gs = self.grad_factor()          # _opt_launch's grad_scale
        if self.dynamic:                 # szn_loss_scale_update changes S at the end of the step: keep what these statistics carry
            self.clip_scale.copy_(self.scale_state[:1])
        L.call("szn_clip_coef", 2 * nl, L.ptr(self.grad_stats), self._clip, gs, L.ptr(self.scale_state), L.ptr(self.clip_state), st)

    def grad_factor(self):
        """what the buffers' elements are multiplied by to give the gradient the update uses, apart from the dynamic loss scale and the
        clip coefficient: 1 / (world x static loss scale), and 1 / A under accum=dict(average=True).  The optimizer launches' grad_scale."""
        return (1.0 / self.world if self.dynamic else 1.0 / (self.world * self._loss_scale0)) * self._accum_scale

    def grad_norms(self):
        """the last step's numbers on the host (a sync; tests and logs): grad_report of grad_stats, clip_state and the scale"""
        if self._clip is None:
            raise L.SznError("TrainStep: grad_norms() on a step built without clip=")
        return grad_report(self.grad_segments, self.grad_stats.cpu().numpy(), self.clip_state.cpu().numpy(),
                           self.grad_factor() / float(self.clip_scale.item()))

    # ---- averaged weights (ema=) --------------------------------------------------------------------------------------------
    @staticmethod
    def _check_ema(cfg):
        """ema= checked on the host (before anything touches a device) -> (decay, every, warmup)"""
        if not isinstance(cfg, dict) or "decay" not in cfg or set(cfg) - {"decay", "every", "warmup"}:
            raise ValueError("TrainStep: ema must be a dict(decay=, every=1, warmup=True), got %r" % (cfg,))
        try:
            decay, every = float(cfg["decay"]), cfg.get("every", 1)
            every = 1 if every is None else every
            whole = int(every) == every
        except (TypeError, ValueError):
            raise ValueError("TrainStep: ema decay must be a number and every an integer (got %r)" % (cfg,))
        if not 0.0 <= decay < 1.0:
            raise ValueError("TrainStep: ema decay must lie in [0, 1), got %r" % (cfg["decay"],))
        if not whole or int(every) < 1:
            raise ValueError("TrainStep: ema every must be an integer >= 1, got %r" % (every,))
        warm = cfg.get("warmup", True)
        return decay, int(every), bool(True if warm is None else warm)

    def reset_ema(self):
        """(re)start the average from the current parameters"""
        if self._ema is None:
            raise L.SznError("TrainStep: reset_ema() on a step built without ema=")
        if self._ema_in:
            raise L.SznError("TrainStep: reset_ema() inside averaged_weights()")
        self.ema_w, self.ema_b = self.flat_w.clone(), self.flat_b.clone()
        self.ema_updates = 0

    def _ema_launch(self, st):
        decay, every, warm = self._ema
        if every > 1 and torch.cuda.is_current_stream_capturing():
            raise ValueError("TrainStep: ema every > 1 cannot be captured into a graph, the host decides which steps update the average")
        if self.nstep % every:
            return
        dyn = L.ptr(self.scale_state) if self.dynamic else None
        for avg, p in ((self.ema_w, self.flat_w), (self.ema_b, self.flat_b)):
            L.call("szn_ema_step", p.numel(), L.ptr(avg), L.ptr(p), decay, every, self.nstep if warm else 0, dyn, st)
        self.ema_updates += 1

    def _ema_swap(self, only=2):
        """exchange parameters and average in place (bit for bit), bring the 16-bit weight image in line with the fp32 buffer now in
        place; the rows behind score_fr's slot (seenmask_score's, the padding) lie outside flat_w and are not touched"""
        self._ema_swapped = 0            # how many of the two exchanges this call has queued
        st = L.stream_ptr()
        for i, (p, avg) in enumerate(((self.flat_w, self.ema_w), (self.flat_b, self.ema_b))):
            if i < only:
                L.call("szn_swap_f32", p.numel(), L.ptr(p), L.ptr(avg), st)
                self._ema_swapped = i + 1
        if self.flat_w_lp is not None:
            # the optimizer kernels round their image with the conversion szn_cast uses: casting the restored masters reproduces it
            L.call("szn_cast", L.SZN_F32, L.dtype_code(self.flat_w_lp.dtype), self.flat_w.numel(), L.ptr(self.flat_w),
                   L.ptr(self.flat_w_lp), st)
        self.eng.mark_dirty()

    @contextlib.contextmanager
    def averaged_weights(self):
        """for the duration of the block the model (flat_w, flat_b, the 16-bit weight image, every image the engine derives) holds the
        averaged weights and ema_w / ema_b the raw iterate: an exact in-place exchange, undone in a `finally`, after which all five
        buffers hold the bits they held before and training continues bit for bit.  Nested entry is a no-op.  No step() inside."""
        if self._ema is None:
            raise L.SznError("TrainStep: averaged_weights() on a step built without ema=")
        if self._ema_in:
            yield
            return
        self._ema_in = True
        self._ema_swapped = 0
        try:
            self._ema_swap()
            yield
        finally:
            try:
                # (an entry that failed half way left weights or biases un-exchanged: both kernels are their own inverse, so the
                # exit exchanges exactly what the entry did)
                self._ema_swap(self._ema_swapped)
            finally:
                self._ema_in = False

    def _ema_names(self):
        names = {id(p): k for k, p in self.model.named_parameters()}
        for p, key, view in self._param_slots():
            yield names[id(p)], key, view

    def ema_state_dict(self):
        """the average with model.state_dict()'s keys and layout; entries outside the flat buffers (frozen layers) are the model's"""
        if self._ema is None:
            raise L.SznError("TrainStep: ema_state_dict() on a step built without ema=")
        sd = {k: v.detach().clone() for k, v in self.model.state_dict().items()}
        w, b = (self.flat_w, self.flat_b) if self._ema_in else (self.ema_w, self.ema_b)
        for name, key, view in self._ema_names():
            sd[name] = view(w if key == "w" else b).clone()
        return sd

    def load_ema_state_dict(self, sd):
        """inverse of ema_state_dict (resume): the flat-buffer entries of `sd` become the average"""
        if self._ema is None:
            raise L.SznError("TrainStep: load_ema_state_dict() on a step built without ema=")
        if self._ema_in:
            raise L.SznError("TrainStep: load_ema_state_dict() inside averaged_weights()")
        for name, key, view in self._ema_names():
            if name not in sd:
                raise L.SznError("TrainStep: the stored average lacks %r" % name)
            view(self.ema_w if key == "w" else self.ema_b).copy_(sd[name].to(self.dev, torch.float32))

    def metrics(self, reset=True):
        """running train metrics from the device histogram (trainer_fcn.py:164)"""
        from .utils import _hist_to_metrics
        h = self.hist[0].cpu().numpy()
        if reset:
            self.hist.zero_()
        return _hist_to_metrics(h)
