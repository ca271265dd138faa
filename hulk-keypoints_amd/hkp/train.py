"""Training step (train.py:32-36 restated for the MI355X path) and data parallelism.

Trainer.step = forward (kernel walk, Trace kept) → fused fp64 loss kernel
(dL/dheat) → backward kernels (net.keypoints_backward) → [RCCL all-reduce of
gradients, bucketed and overlapped with the rest of backward] → Adam
(lr 1e-4, weight_decay 1e-4, train.py:79): the optimizer loop stays a PyTorch
optimizer object as the north star asks; its update is either hkp.optim.FusedAdam
(default: one HIP pass over all parameters) or torch.optim.Adam.

Data parallelism: one process per GPU (torchrun), torch.distributed backend
"nccl" = RCCL over xGMI.  Gradients land in flat per-bucket buffers in the
order backward produces them (fc, layer4, …, stem); as soon as a bucket is
complete its all-reduce is launched asynchronously, so communication of the
late layers overlaps the backward of the early ones.  BatchNorm statistics
stay per rank (standard DDP semantics) unless Trainer(sync_bn=True): then the
BN statistics and the BN backward sums are taken over every rank's shard
(Policy(sync_bn=True), hkp.parallel), and a step equals one step over the
global batch.
Parameters and buffers are broadcast from rank 0 when the Trainer is built
(broadcast_state).
"""
import torch
import torch.distributed as dist

from . import net, ops, parallel
from .optim import FusedAdam


class GradBucketer:
    """Bucketed, overlapped gradient all-reduce (mean over ranks)."""

    def __init__(self, params, bucket_bytes=32 << 20, group=None, last_bucket_bytes=None):
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        # RCCL averages inside the all-reduce (ReduceOp.AVG); gloo has no AVG, so
        # there the sum is scaled by 1/world after the wait
        self.avg_in_collective = self.world > 1 and dist.get_backend(group) == "nccl"
        self.op = dist.ReduceOp.AVG if self.avg_in_collective else dist.ReduceOp.SUM
        # backward produces grads roughly in reverse parameter order; buckets are cut
        # from the END of that order (the stem side), the first of them (the last
        # to fill, its all-reduce exposed after backward) capped at
        # last_bucket_bytes (bucket_bytes / 8 by default): for R34 the tail bucket
        # is layer2 + layer1 + stem (~6 MB) instead of a 23 MB remainder
        if last_bucket_bytes is None:
            last_bucket_bytes = bucket_bytes // 8
        order = list(reversed(list(params)))
        tail_first = []
        cur, cur_bytes, cap = [], 0, last_bucket_bytes
        for p in reversed(order):
            if cur and cur_bytes + p.numel() * 4 > cap:
                tail_first.append(cur)
                cur, cur_bytes, cap = [], 0, bucket_bytes
            cur.insert(0, p)
            cur_bytes += p.numel() * 4
        if cur:
            tail_first.append(cur)
        self.buckets = list(reversed(tail_first))
        self.slot = {}
        self.flat = []
        for bi, ps in enumerate(self.buckets):
            n = sum(p.numel() for p in ps)
            flat = torch.zeros(n, device=ps[0].device, dtype=torch.float32)
            off = 0
            for p in ps:
                self.slot[p] = (bi, off)
                off += p.numel()
            self.flat.append(flat)
        self._reset()

    def _reset(self):
        self.pending = [len(ps) for ps in self.buckets]
        self.works = [None] * len(self.buckets)
        self.streams = [set() for _ in self.buckets]

    def ready(self, p, g):
        """Copy g into its bucket on the CURRENT stream (the one that produced g:
        main, or the side stream a wgrad ran on); a full bucket's all-reduce is
        launched after the current stream joins the other streams that copied
        into it (once per bucket, not per gradient)."""
        bi, off = self.slot[p]
        cur = torch.cuda.current_stream(g.device) if g.is_cuda else None    # (gloo tests: CPU tensors)
        self.flat[bi][off:off + p.numel()].copy_(g.reshape(-1))
        self.streams[bi].add(cur)
        self.pending[bi] -= 1
        if self.pending[bi] == 0:
            for s in self.streams[bi]:
                if s is not None and s != cur:
                    cur.wait_stream(s)
            if self.world > 1:
                self.works[bi] = dist.all_reduce(self.flat[bi], op=self.op, group=self.group, async_op=True)

    def finish(self):
        """Wait for every bucket; average; point p.grad at the flat buffers."""
        if any(self.pending):
            raise RuntimeError("gradient missing for %d parameters" % sum(self.pending))
        for bi, w in enumerate(self.works):
            if w is not None:
                w.wait()
            else:                              # world 1: the copies themselves
                for s in self.streams[bi]:
                    if s is not None and s != torch.cuda.current_stream(s.device):
                        torch.cuda.current_stream(s.device).wait_stream(s)
            if self.world > 1 and not self.avg_in_collective:
                self.flat[bi].mul_(1.0 / self.world)
        for p, (bi, off) in self.slot.items():
            p.grad = self.flat[bi][off:off + p.numel()].view_as(p)
        self._reset()


def broadcast_state(model, src=0, group=None):
    """Copy rank src's parameters and buffers (BN running stats and counters) to
    every rank, in place — what DDP does at construction.  Tensors are flattened
    per dtype into one buffer each, so a whole network costs a few collectives."""
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        return
    tensors = [t.data for t in list(model.parameters()) + list(model.buffers())]
    by_dtype = {}
    for t in tensors:
        by_dtype.setdefault((t.dtype, t.device), []).append(t)
    for (dtype, dev), ts in by_dtype.items():
        flat = torch.cat([t.reshape(-1) for t in ts])
        dist.broadcast(flat, src, group=group)
        off = 0
        for t in ts:
            t.copy_(flat[off:off + t.numel()].view_as(t))
            off += t.numel()


LINES_ROUTES = ("dense", "walk")      # loss_params["lines"]: how line labels reach the loss


class Trainer:
    """One optimizer step per call, reference semantics (train.py:33-36)."""

    def __init__(self, model, lr=1e-4, weight_decay=1e-4, loss="bce", sigma=8.0, distributed=False,
                 bucket_mb=32, optimizer="fused", sync_bn=False, group=None, force_buckets=False, absent="zero",
                 max_grad_norm=None, ema_decay=None, loss_params=None, tags=None):
        """loss: "bce", "mse" or "qfl" (ops.LOSS_KINDS); loss_params: the other keyword
        arguments of ops.heat_loss / ops.heat_loss_multi, e.g. {"beta": 2.0, "norm":
        "instances"} for the quality focal loss (point labels, uv or pts, only).  Under data
        parallelism norm="instances" divides by each rank's own count of present instances,
        as "ignore" does with its active planes: the all-reduced gradient is the mean of the
        per-rank quotients, not the sum over the global batch divided by its instances.
        loss_params may also hold "class_weights", a sequence of K floats, and "topk"
        (ops.heat_loss_planes; point labels only): the loss kernel then gets the plane weights
        class_weights[None, :] * weights, weights [B,K] being forward_backward's per-image
        weights (all one when not given; a weight that is not > 0 marks a plane as not
        labelled), and per image only the topk planes with the largest weighted loss are
        counted.  The class weights are put on the device once.  With either key, or with
        weights passed to a step, trainer.plane_loss and trainer.plane_used are that step's
        device tensors [B,K] (None otherwise); no host synchronisation is added.  A step given
        mask= (uint8 [B,H,W] class bits in the frame of the heatmaps, hkp.masks; point labels
        only, K <= 8) leaves the masked pixels out of the loss (ops.heat_loss_masked) and
        sets trainer.plane_pixels, the kept pixels per plane, next to the other two.  Under data
        parallelism each rank divides by its own divisor (its counted planes or their
        instances), as for "ignore" and "instances" above; the selection is per image, so it
        does not depend on how the batch is sharded.
        max_grad_norm / ema_decay: FusedAdam's options (hkp.optim): clip the gradients
        by their global L2 norm; keep an exponential moving average of the parameters
        (ema_weights() runs a block on it).  Under data parallelism the norm is taken in
        opt.step(), after the bucketed all-reduce: every rank holds the same averaged
        gradients and computes the same coefficient, with no further collective.
        absent: what a plane of multi-instance labels (pts [B,K,M,3]: u, v, flag) without
        a present instance does: "zero" trains it against the all-zero target, "ignore"
        leaves it out of the loss (its gradient is zero, the mean runs over the other
        planes).  Under data parallelism "ignore" divides by each rank's own count of
        active planes, so the all-reduced gradient is the mean of the per-rank means
        (DDP semantics), not the mean over the global batch's active planes.
        sync_bn: BN statistics and their backward sums over every rank of
        `group` (default: the world; the step then equals one step over the
        global batch), instead of per-rank BN (DDP semantics, the default).
        force_buckets: the DP gradient path (bucket copies, stream joins) at world
        size 1, to time its overhead on one GPU.
        tags: None, or a dict {"classes": (class indices), "weight": 1e-3, "pull": 1.0,
        "push": 1.0} — associative-embedding tags (hkp.grouping): the head then runs over
        the fc rows 0..2K-1 (2K <= 16), row K + c being the tag map of class c, and the
        pull / push loss of ops.tag_loss on the stride-8 lattice, times weight (default
        HigherHRNet's 1e-3), adds its gradient to dlow before the fc backward.  Tags need
        pts labels; a step also takes gid int32 [B,K,M], the cable of every slot (None:
        grouping.slot_groups — slot m of each listed class is cable m).  step() still
        returns the heat loss; trainer.tag_loss is the step's device tensor (total, mean
        pull, mean push), None without tags; no host synchronisation is added.  Under data
        parallelism each rank divides by its own batch size, as the other losses do with
        their divisors."""
        self.model = model
        self.tags = self._tags_choice(tags, model.num_keypoints)
        self.tag_loss = None
        self.group = group
        self.sync_bn = sync_bn
        # SyncBN gathers on their own communicator over the same ranks (RCCL orders
        # the collectives of one communicator by issue, so the 33 + 33 per-step R34
        # BN gathers would otherwise wait behind in-flight gradient buckets)
        multi = sync_bn and dist.is_initialized() and dist.get_world_size(group) > 1
        self.bn_group = parallel.new_group_like(group) if multi else group
        # the empty-shard check's host (gloo) group, created here — collectively, on
        # every rank, next to the communicator above — never lazily inside a step
        # (dist.new_group is collective over the default group: ranks outside a
        # subgroup would never make the call)
        if multi:
            parallel.host_group(group)
        self.shard_check = parallel.ShardCheck(group)
        self.policy = model.policy.with_(sync_bn=True, sync_group=self.bn_group) if sync_bn else model.policy
        self.params = list(model.parameters())
        self.loss_kind = loss
        self.loss_params = dict(loss_params or {})
        if set(self.loss_params) - {"beta", "norm", "class_weights", "topk", "lines"}:
            raise ValueError("loss_params may hold beta, norm, class_weights, topk and lines, got %r" % (loss_params,))
        # how a step with line labels reaches the loss: "dense" (ops.line_target, then the
        # dense ops.heat_loss) or "walk" (ops.heat_loss_lines, the target in registers)
        self.lines_route = self.loss_params.pop("lines", "dense")
        if self.lines_route not in LINES_ROUTES:
            raise ValueError("loss_params['lines'] must be one of %s, got %r"
                             % (", ".join(LINES_ROUTES), self.lines_route))
        self.topk = self.loss_params.pop("topk", None)
        ops._planes_choice("Trainer", None, self.topk)
        cw = self.loss_params.pop("class_weights", None)
        if cw is not None:
            cw = [float(v) for v in cw]
            if len(cw) != model.num_keypoints:
                raise ValueError("class_weights must hold %d floats, got %d" % (model.num_keypoints, len(cw)))
        self._class_weights = cw              # the floats; the device tensor is built at the first step
        self.class_weights = None
        self.plane_loss = self.plane_used = self.plane_pixels = None
        self.sigma = sigma
        if absent not in ops.ABSENT_MODES:
            raise ValueError("absent must be one of %s, got %r" % (", ".join(ops.ABSENT_MODES), absent))
        self.absent = absent
        if optimizer not in ("fused", "torch"):
            raise ValueError("optimizer must be 'fused' or 'torch'")
        if optimizer == "fused":
            self.opt = FusedAdam(self.params, lr=lr, weight_decay=weight_decay, max_grad_norm=max_grad_norm,
                                 ema_decay=ema_decay)
        elif max_grad_norm is not None or ema_decay is not None:
            raise ValueError("max_grad_norm / ema_decay need optimizer='fused'")
        else:
            self.opt = torch.optim.Adam(self.params, lr=lr, weight_decay=weight_decay)
        use_dp = distributed and dist.is_initialized() and dist.get_world_size(group) > 1
        if use_dp:
            broadcast_state(model, group=group)   # every replica starts from rank 0's weights and BN buffers
        self.bucketer = GradBucketer(self.params, bucket_mb << 20, group=group) if (use_dp or force_buckets) \
            else None

    @staticmethod
    def _tags_choice(tags, k):
        if tags is None:
            return None
        if not isinstance(tags, dict) or set(tags) - {"classes", "weight", "pull", "push"} or "classes" not in tags:
            raise ValueError("tags must be a dict with classes and optionally weight, pull, push, got %r" % (tags,))
        if 2 * k > 16:
            raise ValueError("tags take the fc rows K..2K-1 of at most 16 head rows: K = %d is too many" % k)
        classes = tuple(tags["classes"])
        for c in classes:
            if isinstance(c, bool) or not isinstance(c, int) or not 0 <= c < k:
                raise ValueError("tags: classes are indices in 0..%d, got %r" % (k - 1, classes))
        if not classes or len(set(classes)) != len(classes):
            raise ValueError("tags: classes %r must name at least one class, none twice" % (classes,))
        out = dict(classes=classes)
        for name, dflt in (("weight", 1e-3), ("pull", 1.0), ("push", 1.0)):
            try:
                out[name] = ops._tag_weight("Trainer(tags)", name, tags.get(name, dflt))
            except ops.HkpError as e:
                raise ValueError(str(e))
        return out

    def _plane_weights(self, weights, device):
        """class_weights[None, :] * weights as the kernel's [B,K] (either may be missing)."""
        if self._class_weights is not None and (self.class_weights is None or self.class_weights.device != device):
            self.class_weights = torch.tensor(self._class_weights, dtype=torch.float32, device=device)
        if weights is None:
            return None if self.class_weights is None else self.class_weights[None, :]
        return weights if self.class_weights is None else self.class_weights[None, :] * weights

    def _lines_choice(self, x, uv, target, pts, lines, planes):
        """The checks of a step with line labels, before the forward; returns the labels the
        target is made from: lines, with the points of pts in front as zero-length segments."""
        from . import lines as L
        who = "Trainer"
        if self.loss_kind not in ("bce", "mse") or self.loss_params.get("norm", "elements") != "elements":
            raise ops.HkpError("%s: lines train through the dense target: loss 'bce' or 'mse' with norm 'elements', "
                               "not %r / %r" % (who, self.loss_kind, self.loss_params.get("norm", "elements")))
        if self.absent != "zero":
            raise ops.HkpError("%s: lines need absent='zero' (a plane without a present segment is a negative)" % who)
        if planes:
            raise ops.HkpError("%s: weights, class_weights, topk and mask are not supported with lines" % who)
        if uv is not None or target is not None:
            raise ops.HkpError("%s: pass lines alone or with pts, not with uv or target" % who)
        ops._lines_shape(lines, who + ".lines")
        nk = (x.shape[0], self.model.num_keypoints)
        if tuple(lines.shape[:2]) != nk:
            raise ops.HkpError("%s: lines %s do not go with %d images of %d classes" % ((who, tuple(lines.shape)) + nk))
        ops._need_lines(lines, who + ".lines")
        if pts is None:
            return lines
        ops._need_pts(pts, who + ".pts")
        return L.concat(L.from_points(pts), lines)

    def _lines_walk_choice(self, x, uv, target, pts, lines, weights, mask):
        """The checks of a step with line labels under loss_params["lines"] = "walk", before
        the forward; returns the labels ops.heat_loss_lines gets: lines, with the points of
        pts in front as zero-length segments."""
        from . import lines as L
        who = "Trainer"
        if uv is not None or target is not None:
            raise ops.HkpError("%s: pass lines alone or with pts, not with uv or target" % who)
        ops._planes_choice(who, weights, self.topk)
        ops._mask_choice(who, mask)
        nk = (x.shape[0], self.model.num_keypoints)
        if mask is not None and nk[1] > 8:
            raise ops.HkpError("%s: a mask holds 8 class bits, the model has K = %d classes" % (who, nk[1]))
        ops._lines_shape(lines, who + ".lines")
        if tuple(lines.shape[:2]) != nk:
            raise ops.HkpError("%s: lines %s do not go with %d images of %d classes" % ((who, tuple(lines.shape)) + nk))
        ops._need_lines(lines, who + ".lines")
        if pts is None:
            return lines
        ops._need_pts(pts, who + ".pts")
        return L.concat(L.from_points(pts), lines)

    def forward_backward(self, x, uv=None, target=None, global_batch=None, pts=None, weights=None, gid=None,
                         mask=None, lines=None):
        """Labels: uv [B,K,2], a dense target [B,K,H,W] (fp64), or pts [B,K,M,3] (u, v,
        flag: the multi-instance target, absent planes per Trainer(absent=...)).
        lines: float32 [B,K,S,5] line labels (hkp.lines), alone or with pts: the heat target
        is ops.line_target of the segments, the points of pts among them as zero-length
        segments, and the loss is the dense ops.heat_loss against it.  "bce" / "mse" and
        absent="zero" only; no weights, class_weights, topk or mask; tags read pts alone.
        Under Trainer(loss_params={"lines": "walk"}) the same labels go to ops.heat_loss_lines
        in one call, without a dense target, and every choice of the point path holds: "qfl"
        with beta, norm, absent="ignore", class_weights, topk, weights and mask, with
        plane_loss / plane_used / plane_pixels filled as there.
        weights: float32 [B,K] per-image plane weights (point labels only; see __init__).
        gid: int32 [B,K,M], Trainer(tags=...) only: the group of every slot of pts.
        global_batch (SyncBN): the job's batch size — the same on every rank, x
        being this rank's hkp.parallel.shard_range share of it; lets the empty-shard
        guard run without a host collective (parallel.ShardCheck)."""
        if self.sync_bn:
            self.shard_check(x.shape[0], global_batch)
        m = self.model
        planes = weights is not None or self._class_weights is not None or self.topk is not None or mask is not None
        self.plane_loss = self.plane_used = self.plane_pixels = None
        walk = lines is not None and self.lines_route == "walk"
        if planes and not walk:                # checked before the forward
            if target is not None or (pts is None) == (uv is None):
                raise ops.HkpError("Trainer: class_weights, topk, weights and mask need pts or uv labels alone; a "
                                   "dense target is not supported")
            ops._planes_choice("Trainer", weights, self.topk)
            ops._mask_choice("Trainer", mask)
            if mask is not None and m.num_keypoints > 8:
                raise ops.HkpError("Trainer: a mask holds 8 class bits, the model has K = %d classes"
                                   % m.num_keypoints)
        self.tag_loss = None
        if self.tags is None:
            if gid is not None:
                raise ops.HkpError("Trainer: gid goes with Trainer(tags=...)")
        elif pts is None or uv is not None or target is not None:      # checked before the forward
            raise ops.HkpError("Trainer: tags need pts labels alone; uv and a dense target carry no groups")
        if walk:
            lab_lines = self._lines_walk_choice(x, uv, target, pts, lines, weights, mask)
        else:
            lab_lines = None if lines is None else self._lines_choice(x, uv, target, pts, lines, planes)
        trace = net.Trace(self.policy)
        kw = {} if self.tags is None else {"tags": True}           # tags off: the call as it always was
        hm, _, low = net.keypoints_forward(m.resnet.net, x, m.num_keypoints, heat=True, trace=trace, **kw)
        if walk:
            w = self._plane_weights(weights, hm.device)
            if w is not None:
                w = w.expand(hm.shape[0], hm.shape[1]).contiguous()
            loss, dheat, self.plane_loss, self.plane_used, self.plane_pixels = ops.heat_loss_lines(
                hm, lab_lines, self.sigma, self.loss_kind, self.absent, want_grad=True, weights=w, topk=self.topk,
                mask=mask, **self.loss_params)
        elif lab_lines is not None:
            tgt, _ = ops.line_target(lab_lines, hm.shape[2], hm.shape[3], self.sigma)
            loss, dheat = ops.heat_loss(hm, tgt, None, self.sigma, self.loss_kind, want_grad=True)
        elif planes:
            w = self._plane_weights(weights, hm.device)
            if w is not None:
                w = w.expand(hm.shape[0], hm.shape[1]).contiguous()
            lab, absent = (pts, self.absent) if pts is not None else (ops._uv_as_pts(hm, uv), "zero")
            if mask is not None:
                loss, dheat, self.plane_loss, self.plane_used, self.plane_pixels = ops.heat_loss_masked(
                    hm, lab, mask, self.sigma, self.loss_kind, absent, want_grad=True, weights=w, topk=self.topk,
                    **self.loss_params)
            else:
                loss, dheat, self.plane_loss, self.plane_used = ops.heat_loss_planes(
                    hm, lab, self.sigma, self.loss_kind, absent, want_grad=True, weights=w, topk=self.topk,
                    **self.loss_params)
        elif pts is not None:
            if uv is not None or target is not None:
                raise ops.HkpError("Trainer: pass pts alone, not with uv or target")
            loss, dheat = ops.heat_loss_multi(hm, pts, self.sigma, self.loss_kind, self.absent, want_grad=True,
                                              **self.loss_params)
        else:
            loss, dheat = ops.heat_loss(hm, target, uv, self.sigma, self.loss_kind, want_grad=True,
                                        **self.loss_params)
        grads = net.Grads(on_ready=self.bucketer.ready if self.bucketer else None)
        if self.tags is None:
            net.keypoints_backward(m.resnet.net, trace, dheat, grads)
        else:
            tg = self.tags
            if gid is None:
                from .grouping import slot_groups
                gid = slot_groups(pts.shape[0], pts.shape[1], pts.shape[2], tg["classes"], pts.device)
            self.tag_loss, dtag = ops.tag_loss(low, pts, gid, hm.shape[2], hm.shape[3], tg["weight"], tg["pull"],
                                               tg["push"])
            net.keypoints_backward(m.resnet.net, trace, dheat, grads, dtag=dtag)
        if self.bucketer is not None:
            self.bucketer.finish()
        else:
            for p in self.params:
                p.grad = grads[p]
        return loss

    def step(self, x, uv=None, target=None, global_batch=None, pts=None, weights=None, gid=None, mask=None,
             lines=None):
        if lines is not None:
            loss = self.forward_backward(x, uv, target, global_batch, pts=pts, weights=weights, gid=gid, mask=mask,
                                         lines=lines)
        elif mask is None:                     # the call as it always was
            loss = self.forward_backward(x, uv, target, global_batch, pts=pts, weights=weights, gid=gid)
        else:
            loss = self.forward_backward(x, uv, target, global_batch, pts=pts, weights=weights, gid=gid, mask=mask)
        self.opt.step()
        return loss

    def ema_weights(self):
        """Context manager: the model's parameters are their EMA inside the block
        (FusedAdam.ema_weights)."""
        return self.opt.ema_weights()
