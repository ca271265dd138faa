"""autograd bridge: the whole keypoint network is ONE torch.autograd.Function.

forward runs hkp.net's kernel walk keeping a Trace of the activations the
backward needs; backward runs the hand-written backward kernels and returns
every parameter gradient at once.  This is what makes the reference's
training idiom (train.py:21,25,35: ``model.forward(img).double()`` →
``nn.BCELoss()`` → ``loss.backward()``) work unchanged on this path.

HeatmapLoss is the fused fp64 BCE/MSE (train.py:25 / :13) as a Function too, and the
quality focal loss (kind="qfl", not in the reference) goes the same way.
"""
import torch

from . import net, ops


class _KeypointsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, model, *params):
        trace = net.Trace(model.policy)
        hm, _, _ = net.keypoints_forward(model.resnet.net, x, model.num_keypoints, heat=True, trace=trace)
        ctx.trace, ctx.model = trace, model
        return hm

    @staticmethod
    def backward(ctx, d_heat):
        model = ctx.model
        # model.grad_ready (DP: GradBucketer.ready) sees each gradient as soon as it
        # exists, so bucket all-reduces overlap the rest of this backward
        grads = net.keypoints_backward(model.resnet.net, ctx.trace, d_heat.contiguous(),
                                       net.Grads(on_ready=getattr(model, "grad_ready", None)))
        ctx.trace = None
        out = [None, None]
        for p in model.parameters():
            out.append(grads.get(p))
        return tuple(out)


def keypoints_heatmaps(model, x):
    return _KeypointsFn.apply(x, model, *model.parameters())


def _loss_extras(kind, beta, norm):
    """beta / norm as keyword arguments for ops, none at all for the reference's losses
    with their defaults (those calls stay what they were)."""
    return {"beta": beta, "norm": norm} if (kind == "qfl" or norm != "elements") else {}


class _HeatLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, heat, target, uv, sigma, kind, beta, norm):
        loss, dheat = ops.heat_loss(heat.contiguous(), target, uv, sigma, kind,
                                    want_grad=torch.is_grad_enabled() or heat.requires_grad,
                                    **_loss_extras(kind, beta, norm))
        ctx.save_for_backward(dheat)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dheat,) = ctx.saved_tensors
        return dheat * g.to(dheat.dtype), None, None, None, None, None, None


class _HeatLossMultiFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, heat, pts, sigma, kind, absent, beta, norm):
        loss, dheat = ops.heat_loss_multi(heat.contiguous(), pts, sigma, kind, absent,
                                          want_grad=torch.is_grad_enabled() or heat.requires_grad,
                                          **_loss_extras(kind, beta, norm))
        ctx.save_for_backward(dheat)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dheat,) = ctx.saved_tensors
        return dheat * g.to(dheat.dtype), None, None, None, None, None, None


class _HeatLossPlanesFn(torch.autograd.Function):
    """ops.heat_loss_planes; the per-plane values leave as non-differentiable outputs."""

    @staticmethod
    def forward(ctx, heat, pts, sigma, kind, absent, beta, norm, weights, topk):
        loss, dheat, plane_loss, plane_used = ops.heat_loss_planes(
            heat.contiguous(), pts, sigma, kind, absent, want_grad=torch.is_grad_enabled() or heat.requires_grad,
            beta=beta, norm=norm, weights=weights, topk=topk)
        ctx.save_for_backward(dheat)
        ctx.mark_non_differentiable(plane_loss, plane_used)
        return loss, plane_loss, plane_used

    @staticmethod
    def backward(ctx, g, _gl, _gu):
        (dheat,) = ctx.saved_tensors
        return (dheat * g.to(dheat.dtype),) + (None,) * 8


class _HeatLossMaskedFn(torch.autograd.Function):
    """ops.heat_loss_masked (heat_loss_planes with a per-pixel ignore mask); the per-plane
    values leave as non-differentiable outputs."""

    @staticmethod
    def forward(ctx, heat, pts, sigma, kind, absent, beta, norm, weights, topk, mask):
        loss, dheat, plane_loss, plane_used, plane_pixels = ops.heat_loss_masked(
            heat.contiguous(), pts, mask, sigma, kind, absent,
            want_grad=torch.is_grad_enabled() or heat.requires_grad, beta=beta, norm=norm, weights=weights, topk=topk)
        ctx.save_for_backward(dheat)
        ctx.mark_non_differentiable(plane_loss, plane_used, plane_pixels)
        return loss, plane_loss, plane_used, plane_pixels

    @staticmethod
    def backward(ctx, g, _gl, _gu, _gp):
        (dheat,) = ctx.saved_tensors
        return (dheat * g.to(dheat.dtype),) + (None,) * 9


def heatmap_loss(heat, target=None, uv=None, sigma=8.0, kind="bce", pts=None, absent="zero", beta=2.0,
                 norm="elements", weights=None, topk=None, return_planes=False, mask=None, lines=None):
    """mean BCE (default) or MSE between fp32 heatmaps and the fp64 Gaussian target
    (dense ``target`` or recomputed from ``uv``), returned as a 0-dim fp64 tensor.
    ``pts`` [N,K,M,3] (u, v, flag) in place of both: the multi-instance target
    (ops.heat_loss_multi), planes without a present instance handled per ``absent``
    ("zero": negatives; "ignore": left out of the mean).
    ``kind="qfl"`` (``uv`` or ``pts`` labels): the quality focal loss, BCE against the
    soft target scaled by |target - heat|^``beta`` per pixel; ``norm="instances"``
    divides the sum by the number of present instances instead of taking the mean.
    ``weights`` float32 [N,K], ``topk`` and ``return_planes`` (``uv`` or ``pts`` labels):
    ops.heat_loss_planes: a weight per (image, class) plane (not > 0: the plane is not
    labelled and leaves the loss), per image only the ``topk`` planes with the largest
    weighted loss, and with ``return_planes`` the result is (loss, plane_loss [N,K] f64,
    plane_used [N,K] int32), the two extras detached.
    ``mask`` uint8 [N,H,W] (``uv`` or ``pts`` labels, K <= 8): the per-pixel ignore mask of
    ops.heat_loss_masked, bit c of a byte taking that pixel out for class c; with
    ``return_planes`` a fourth value follows, plane_pixels [N,K] int32.
    ``lines`` float32 [N,K,S,5] (hkp.lines), alone or with ``pts``: the dense target is
    ops.line_target of the segments, the points of ``pts`` among them as zero-length
    segments; "bce" / "mse", ``absent="zero"`` and ``norm="elements"`` only, and none of
    ``weights``, ``topk``, ``return_planes``, ``mask``, ``uv`` or ``target``."""
    if lines is not None:
        from . import lines as L
        if kind not in ("bce", "mse") or norm != "elements" or absent != "zero":
            raise ops.HkpError("heatmap_loss: lines train through the dense target: kind 'bce' or 'mse', norm "
                               "'elements' and absent 'zero', not %r / %r / %r" % (kind, norm, absent))
        if weights is not None or topk is not None or return_planes or mask is not None:
            raise ops.HkpError("heatmap_loss: weights, topk, return_planes and mask are not supported with lines")
        if uv is not None or target is not None:
            raise ops.HkpError("heatmap_loss: pass lines alone or with pts, not with uv or target")
        if not isinstance(heat, torch.Tensor) or heat.dim() != 4:
            raise ops.HkpError("heatmap_loss: heat must be a tensor [N,K,H,W]")
        ops._lines_shape(lines, "heatmap_loss.lines")
        if tuple(lines.shape[:2]) != tuple(heat.shape[:2]):
            raise ops.HkpError("heatmap_loss: lines %s do not go with heat %s" % (tuple(lines.shape), tuple(heat.shape)))
        ops._need_lines(lines, "heatmap_loss.lines")
        if pts is not None:
            ops._need_pts(pts, "heatmap_loss.pts")
            lines = L.concat(L.from_points(pts), lines)
        tgt, _ = ops.line_target(lines, heat.shape[2], heat.shape[3], sigma)
        return _HeatLossFn.apply(heat, tgt, None, sigma, kind, beta, norm)
    if mask is not None:
        if target is not None or (pts is None) == (uv is None):
            raise ops.HkpError("heatmap_loss: a mask needs pts or uv labels alone; a dense target is not supported")
        ops._loss_choice("heatmap_loss", kind, norm, beta)
        ops._planes_choice("heatmap_loss", weights, topk, heat)
        ops._mask_choice("heatmap_loss", mask, heat)
        if pts is None:
            pts, absent = ops._uv_as_pts(heat, uv), "zero"
        out = _HeatLossMaskedFn.apply(heat, pts, sigma, kind, absent, beta, norm, weights, topk, mask)
        return out if return_planes else out[0]
    if weights is not None or topk is not None or return_planes:
        if target is not None or (pts is None) == (uv is None):
            raise ops.HkpError("heatmap_loss: weights, topk and return_planes need pts or uv labels alone; a dense "
                               "target is not supported")
        ops._loss_choice("heatmap_loss", kind, norm, beta)
        ops._planes_choice("heatmap_loss", weights, topk, heat)
        if pts is None:
            pts, absent = ops._uv_as_pts(heat, uv), "zero"
        loss, plane_loss, plane_used = _HeatLossPlanesFn.apply(heat, pts, sigma, kind, absent, beta, norm, weights,
                                                               topk)
        return (loss, plane_loss, plane_used) if return_planes else loss
    if pts is not None:
        if target is not None or uv is not None:
            raise ops.HkpError("heatmap_loss: pass pts alone, not with target or uv")
        return _HeatLossMultiFn.apply(heat, pts, sigma, kind, absent, beta, norm)
    return _HeatLossFn.apply(heat, target, uv, sigma, kind, beta, norm)


class _HeatLossLinesFn(torch.autograd.Function):
    """ops.heat_loss_lines; the per-plane values leave as non-differentiable outputs
    (plane_pixels is None without a mask)."""

    @staticmethod
    def forward(ctx, heat, lines, sigma, kind, absent, beta, norm, weights, topk, mask):
        loss, dheat, plane_loss, plane_used, plane_pixels = ops.heat_loss_lines(
            heat.contiguous(), lines, sigma, kind, absent, want_grad=torch.is_grad_enabled() or heat.requires_grad,
            beta=beta, norm=norm, weights=weights, topk=topk, mask=mask)
        ctx.save_for_backward(dheat)
        if plane_pixels is None:
            ctx.mark_non_differentiable(plane_loss, plane_used)
        else:
            ctx.mark_non_differentiable(plane_loss, plane_used, plane_pixels)
        return loss, plane_loss, plane_used, plane_pixels

    @staticmethod
    def backward(ctx, g, _gl, _gu, _gp):
        (dheat,) = ctx.saved_tensors
        return (dheat * g.to(dheat.dtype),) + (None,) * 9


def line_heatmap_loss(heat, lines, sigma=8.0, kind="bce", absent="zero", *, pts=None, beta=2.0, norm="elements",
                      weights=None, topk=None, mask=None, return_planes=False):
    """The heatmap loss against line labels without the dense target (ops.heat_loss_lines):
    ``lines`` float32 [N,K,S,5] (hkp.lines), and with ``pts`` [N,K,M,3] the labels are
    lines.concat(lines.from_points(pts), lines), the points as zero-length segments.
    Every choice of the point losses holds: ``kind`` "bce" / "mse" / "qfl" with ``beta``,
    ``absent``, ``norm`` ("instances" counts present segment slots, points and pieces
    alike), ``weights`` float32 [N,K], ``topk`` and ``mask`` uint8 [N,H,W] (K <= 8).  The
    result is a 0-dim fp64 tensor; with ``return_planes`` it is (loss, plane_loss [N,K] f64,
    plane_used [N,K] int32), and with a mask a fourth value, plane_pixels [N,K] int32, the
    extras detached.  heatmap_loss(lines=) keeps its dense route and its limits."""
    from . import lines as L
    ops._loss_choice("line_heatmap_loss", kind, norm, beta)
    if absent not in ops.ABSENT_MODES:
        raise ops.HkpError("line_heatmap_loss: unknown absent %r (known: %s)" % (absent, ", ".join(ops.ABSENT_MODES)))
    ops._planes_choice("line_heatmap_loss", weights, topk, heat)
    ops._mask_choice("line_heatmap_loss", mask, heat)
    if not isinstance(heat, torch.Tensor) or heat.dim() != 4:
        raise ops.HkpError("line_heatmap_loss: heat must be a tensor [N,K,H,W]")
    ops._lines_shape(lines, "line_heatmap_loss.lines")
    if tuple(lines.shape[:2]) != tuple(heat.shape[:2]):
        raise ops.HkpError("line_heatmap_loss: lines %s do not go with heat %s"
                           % (tuple(lines.shape), tuple(heat.shape)))
    if pts is not None:
        if not isinstance(pts, torch.Tensor) or pts.dim() != 4 or pts.shape[3] != 3 \
                or tuple(pts.shape[:2]) != tuple(heat.shape[:2]):
            raise ops.HkpError("line_heatmap_loss: pts must be [N,K,M,3] with heat's N and K, got %s"
                               % (tuple(pts.shape) if isinstance(pts, torch.Tensor) else type(pts).__name__,))
        if pts.shape[2] + lines.shape[2] > L.HKP_LINE_MAX_S:
            raise ops.HkpError("line_heatmap_loss: %d points and %d segments a plane, at most %d slots together"
                               % (pts.shape[2], lines.shape[2], L.HKP_LINE_MAX_S))
    ops._need_lines(lines, "line_heatmap_loss.lines")
    if pts is not None:
        ops._need_pts(pts, "line_heatmap_loss.pts")
        lines = L.concat(L.from_points(pts), lines)
    out = _HeatLossLinesFn.apply(heat, lines, sigma, kind, absent, beta, norm, weights, topk, mask)
    if not return_planes:
        return out[0]
    return out if mask is not None else out[:3]


class HeatmapBCELoss(torch.nn.Module):
    """Drop-in for ``nn.BCELoss()(pred.double(), gt)`` (train.py:25) on GPU heatmaps."""

    def forward(self, pred, gt):
        if pred.dtype == torch.float64:
            raise TypeError("pass the fp32 heatmaps (the kernel performs the .double() itself)")
        return heatmap_loss(pred, target=gt, kind="bce")


class HeatmapMSELoss(torch.nn.Module):
    def forward(self, pred, gt):
        return heatmap_loss(pred, target=gt, kind="mse")
