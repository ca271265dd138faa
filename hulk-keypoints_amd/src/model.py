"""MI355X-native restatement of src/model.py (KeypointsGauss, :10-22).

``forward(x)`` returns sigmoid heatmaps [B,K,H,W] exactly like the reference,
computed by the fused K-channel head (only the K kept fc rows are evaluated;
SURVEY D8).  Autograd flows through it (train.py:21,35 call pattern) via one
autograd.Function that runs the hand-written backward kernels.
``backbone`` selects resnet18 / resnet34 (default, the reference) / resnet50.
``precision`` (or a whole hkp.policy.Policy as ``policy``) selects the conv
arithmetic: "f16x3" (default, fp32-accurate), "fp32" (exact) or "f16" (config
C4, inference only); it is per model, not process-global.
"""
import torch
import torch.nn as nn

from hkp import autograd as hkp_autograd
from hkp import net
from hkp.policy import DEFAULT
from src.resnet_dilated import ResnetDilated8s


class KeypointsGauss(nn.Module):
    def __init__(self, num_keypoints, img_height=480, img_width=640, backbone="resnet34", pretrained=True,
                 precision=None, policy=None):
        super().__init__()
        if policy is None:
            policy = DEFAULT if precision is None else DEFAULT.with_(precision=precision)
        elif precision is not None:
            policy = policy.with_(precision=precision)
        self.num_keypoints = num_keypoints
        self.num_outputs = self.num_keypoints
        self.img_height = img_height
        self.img_width = img_width
        self.resnet = ResnetDilated8s(backbone, pretrained=pretrained, policy=policy)
        self.sigmoid = torch.nn.Sigmoid()
        # DP training through autograd (train.py): called as grad_ready(param, grad)
        # for each gradient as the backward kernels produce it (GradBucketer.ready)
        self.grad_ready = None

    @property
    def policy(self):
        return self.resnet.policy

    @policy.setter
    def policy(self, p):
        self.resnet.policy = p

    def forward(self, x):
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            return hkp_autograd.keypoints_heatmaps(self, x)
        hm, _, _ = net.keypoints_forward(self.resnet.net, x, self.num_keypoints, heat=True, argmax=False,
                                         pol=self.policy)
        return hm

    @torch.no_grad()
    def predict_keypoints(self, x, policy=None):
        """Fused decode: argmax (y, x) int32 [B,K,2] without materialising the heatmap
        (src/prediction.py:46 semantics, first max wins)."""
        _, yx, _ = net.keypoints_forward(self.resnet.net, x, self.num_keypoints, heat=False, argmax=True,
                                         pol=policy or self.policy)
        return yx

    @torch.no_grad()
    def lowres_logits(self, x, tta=None, policy=None):
        """The low-res logits [B,K,h,w] fp32 the peak decode reads (not in the
        reference).  tta=None: those of one forward.  tta: a
        hkp.tta.TestTimeAugmentation — one forward per view, in the views' order
        (view 0 is x itself), then one launch that merges them on x's own lattice
        (ops.logits_merge).  Every view is a forward like any other: in train-mode
        BN it takes its own batch statistics and moves the running ones; under
        eval() nothing is written.  Scaled views need a uint8 NHWC batch."""
        pol = policy or self.policy

        def fwd(xv):
            return net.keypoints_forward(self.resnet.net, xv, self.num_keypoints, heat=False, argmax=False, pol=pol,
                                         upsample=False)[2]
        if tta is None:
            return fwd(x)
        tta.check_input(x)
        return tta.run(x, fwd)

    @torch.no_grad()
    def predict_peaks(self, x, max_peaks=4, radius=1, threshold=0.0, policy=None, tta=None):
        """Multi-peak decode (not in the reference): (peaks float32 [B,K,max_peaks,3],
        counts int32 [B,K]) — per heatmap the up to max_peaks best local maxima with
        score >= threshold, best first, no two within Chebyshev distance `radius` of
        each other on the stride-8 lattice, each as (x, y, score): (x, y) like
        soft_argmax and the labels, NOT (y, x) like predict_keypoints; sub-lattice
        positions in input pixels, score the heatmap's value at the node; unused
        slots (-1, -1, 0).  Same inputs as predict_keypoints (fp32 NCHW or uint8
        NHWC); decoded from the low-res logits (ops.heat_peaks): no heatmap is
        allocated and no upsample launch is made.  tta: a
        hkp.tta.TestTimeAugmentation — the peaks of the merged views' logits
        (lowres_logits), in x's own pixels."""
        from hkp import ops
        low = self.lowres_logits(x, tta=tta, policy=policy)
        H, W = net.image_nchw_shape(x)[2:]
        return ops.heat_peaks(low, H, W, max_peaks=max_peaks, radius=radius, threshold=threshold)

    @torch.no_grad()
    def predict_groups(self, x, classes, max_peaks=4, radius=1, threshold=0.0, max_dist=1.0, policy=None):
        """Which peaks belong to one cable (associative-embedding tags, not in the
        reference; a model trained with Trainer(tags=...)): (peaks float32
        [B,K,max_peaks,3], counts int32 [B,K], group int32 [B,K,max_peaks], tag float32
        [B,K,max_peaks]).  One forward over the fc rows 0..2K-1 (2K <= 16), then
        ops.heat_peaks on a contiguous copy of the heat channels — peaks and counts are
        predict_peaks' — then ops.peaks_group: the peaks of `classes` (class indices, taken
        in that order, each class best peak first) grouped greedily by the tag map's value
        at the peak, within max_dist of a group's mean tag; -1 for unused slots and other
        classes.  tta= is not offered: tags are not merged across views (a view's tags are
        its own arbitrary numbers)."""
        from hkp import ops
        k = self.num_keypoints
        low_all = net.keypoints_forward(self.resnet.net, x, k, heat=False, argmax=False, pol=policy or self.policy,
                                        upsample=False, tags=True)[2]
        H, W = net.image_nchw_shape(x)[2:]
        peaks, counts = ops.heat_peaks(low_all[:, :k].contiguous(), H, W, max_peaks=max_peaks, radius=radius,
                                       threshold=threshold)
        group, tag, _ = ops.peaks_group(peaks, counts, low_all, H, W, classes, max_dist=max_dist)
        return peaks, counts, group, tag

    @torch.no_grad()
    def evaluate(self, x, labels, metrics, max_peaks=4, radius=1, threshold=0.0, policy=None, tta=None, mask=None):
        """predict_peaks, then one launch that matches the peaks to `labels` ([B,K,M,3]
        (u, v, flag) or [B,K,2], in input pixels, on the device) and adds the outcome
        into `metrics` (hkp.metrics.KeypointMetrics); no host synchronisation.
        Returns the (peaks, counts) of predict_peaks.  tta: as for predict_peaks.
        mask uint8 [B,H,W] (hkp.masks, in input pixels): the peaks on ignored pixels are left
        out of the match (KeypointMetrics.update(mask=)); what is returned is unfiltered."""
        peaks, counts = self.predict_peaks(x, max_peaks=max_peaks, radius=radius, threshold=threshold, policy=policy,
                                           tta=tta)
        if mask is None:
            metrics.update(peaks, counts, labels)
        else:
            metrics.update(peaks, counts, labels, mask=mask)
        return peaks, counts

    @torch.no_grad()
    def heatmaps_and_keypoints(self, x, policy=None):
        hm, yx, _ = net.keypoints_forward(self.resnet.net, x, self.num_keypoints, heat=True, argmax=True,
                                          pol=policy or self.policy)
        return hm, yx
