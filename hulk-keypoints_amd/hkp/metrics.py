"""Keypoint evaluation that stays on the device (not in the reference).

KeypointMetrics owns the two int64 accumulators of hkp_peaks_match
(include/hulkkp.h): hist [K, T, 2, bins], the score histograms of the true and
false positives per class and threshold, and totals [K, 8].  update() is one
launch and no synchronisation; the host reads the accumulators once, in
compute(), and derives every figure from the integers alone, in float64:
PCK / recall, precision, average precision over the score (COCO's 101-point
interpolation on the binned scores), false alarms on absent keypoints and the
mean localisation error.  Thresholds are distances in pixels of the frame the
labels are given in.  Integer sums do not depend on their order, so merge() and
all_reduce() give the integers of one pass over all the data, exactly.
"""
import numpy as np
import torch

from . import ops
from ._lib import HkpError

RECALL_POINTS = np.linspace(0.0, 1.0, 101)      # COCO's recall thresholds
# totals[c][...] (include/hulkkp.h)
T_PLANES, T_ABSENT, T_INSTANCES, T_PEAKS, T_MATCHED, T_DIST_Q16, T_ABSENT_PEAKS = range(7)


def _ratio(a, b):
    return float(a) / float(b) if b else float("nan")


def average_precision(tp_hist, fp_hist, instances):
    """AP of one class at one threshold from its score histograms (int arrays [bins],
    bin 0 the lowest score): the bins are swept from the highest score down, every
    non-empty bin is one (recall, precision) point, precision is made monotone from
    the right, and the result is the mean precision at the recalls 0, 0.01, .., 1
    (0 where the recall is never reached).  nan without instances."""
    if instances <= 0:
        return float("nan")
    tp = np.asarray(tp_hist, dtype=np.int64)[::-1]
    fp = np.asarray(fp_hist, dtype=np.int64)[::-1]
    keep = (tp + fp) > 0
    ctp = np.cumsum(tp)[keep].astype(np.float64)
    cfp = np.cumsum(fp)[keep].astype(np.float64)
    if ctp.size == 0:
        return 0.0
    recall = ctp / float(instances)
    precision = ctp / (ctp + cfp)
    precision = np.maximum.accumulate(precision[::-1])[::-1]
    idx = np.searchsorted(recall, RECALL_POINTS, side="left")
    q = np.zeros(RECALL_POINTS.size, dtype=np.float64)
    ok = idx < recall.size
    q[ok] = precision[idx[ok]]
    return float(q.mean())


def compute_from_state(hist, totals, thresholds):
    """The metrics dict of KeypointMetrics.compute() from the two integer arrays."""
    hist = np.asarray(hist, dtype=np.int64)
    totals = np.asarray(totals, dtype=np.int64)
    K, T = hist.shape[:2]
    if len(thresholds) != T or totals.shape != (K, 8) or hist.shape[2] != 2:
        raise ValueError("compute_from_state: hist %s, totals %s and %d thresholds do not go together"
                         % (hist.shape, totals.shape, len(thresholds)))
    tp = hist[:, :, 0, :].sum(axis=2)           # [K, T]
    fp = hist[:, :, 1, :].sum(axis=2)
    per_class = []
    aps = []
    for c in range(K):
        inst = int(totals[c, T_INSTANCES])
        ap = [average_precision(hist[c, ti, 0], hist[c, ti, 1], inst) for ti in range(T)]
        if inst > 0:
            aps.extend(ap)
        per_class.append({
            "planes": int(totals[c, T_PLANES]),
            "instances": inst,
            "peaks": int(totals[c, T_PEAKS]),
            "absent_planes": int(totals[c, T_ABSENT]),
            "absent_false_alarms": int(totals[c, T_ABSENT_PEAKS]),
            "true_positives": [int(v) for v in tp[c]],
            "false_positives": [int(v) for v in fp[c]],
            "recall": [_ratio(tp[c, ti], inst) for ti in range(T)],
            "precision": [_ratio(tp[c, ti], tp[c, ti] + fp[c, ti]) for ti in range(T)],
            "ap": ap,
            "mean_error_px": _ratio(float(totals[c, T_DIST_Q16]) / 65536.0, totals[c, T_MATCHED]),
        })
    tot = totals.sum(axis=0)
    overall = {
        "mAP": float(np.mean(aps)) if aps else float("nan"),
        "recall": [_ratio(tp[:, ti].sum(), tot[T_INSTANCES]) for ti in range(T)],
        "precision": [_ratio(tp[:, ti].sum(), tp[:, ti].sum() + fp[:, ti].sum()) for ti in range(T)],
        "mean_error_px": _ratio(float(tot[T_DIST_Q16]) / 65536.0, tot[T_MATCHED]),
        "planes": int(tot[T_PLANES]),
        "instances": int(tot[T_INSTANCES]),
        "peaks": int(tot[T_PEAKS]),
        "absent_planes": int(tot[T_ABSENT]),
        "absent_false_alarms": int(tot[T_ABSENT_PEAKS]),
    }
    return {"thresholds": [float(v) for v in thresholds], "bins": int(hist.shape[3]), "per_class": per_class,
            "overall": overall}


EVAL_KEYS = ("thresholds", "bins", "max_peaks", "radius", "threshold", "tta")


def from_config(cfg, num_keypoints, device=None):
    """config.EVAL (a dict with any of EVAL_KEYS) → (KeypointMetrics, the keyword
    arguments of KeypointsGauss.predict_peaks).  With "tta" (a dict of
    hkp.tta.TestTimeAugmentation's keyword arguments) they hold the object as
    "tta"; without it there is no such entry."""
    unknown = sorted(set(cfg) - set(EVAL_KEYS))
    if unknown:
        raise ValueError("EVAL: unknown keys %s (known: %s)" % (unknown, ", ".join(EVAL_KEYS)))
    if cfg.get("tta") is not None:
        from .tta import from_config as tta_from_config
        metrics, peak_kw = from_config({k: v for k, v in cfg.items() if k != "tta"}, num_keypoints, device)
        peak_kw["tta"] = tta_from_config(cfg["tta"])
        return metrics, peak_kw
    metrics = KeypointMetrics(num_keypoints, cfg.get("thresholds", (2, 4, 8, 16)), bins=cfg.get("bins", 1024),
                              device=device)
    peak_kw = {"max_peaks": int(cfg.get("max_peaks", 4)), "radius": int(cfg.get("radius", 1)),
               "threshold": float(cfg.get("threshold", 0.0))}
    return metrics, peak_kw


def load_labels(path, num_keypoints):
    """One label file as float32 [K, m, 3] (u, v, flag), read as
    KeypointsDataset(instances=...) reads it: [K,2] (every keypoint present once),
    [K,3] or [K,m,3] with 1 <= m <= 16."""
    K = int(num_keypoints)
    a = np.load(path)
    if a.shape == (K, 2):
        a = np.concatenate([a, np.ones((K, 1), dtype=a.dtype)], 1)[:, None, :]
    elif a.shape == (K, 3):
        a = a[:, None, :]
    if a.ndim != 3 or a.shape[0] != K or a.shape[2] != 3 or not 1 <= a.shape[1] <= 16:
        raise ValueError("%s: expected labels [%d,2], [%d,3] or [%d,m,3] with m <= 16, got %s"
                         % (path, K, K, K, a.shape))
    return np.ascontiguousarray(a, dtype=np.float32)


class KeypointMetrics:
    """Accumulates hkp_peaks_match over a validation pass; see the module docstring.
    device=None: the current CUDA device at the first update() (the accumulators
    are host tensors until then, so state / merge / compute work without a GPU)."""

    def __init__(self, num_keypoints, thresholds=(2, 4, 8, 16), bins=1024, device=None):
        self.num_keypoints = int(num_keypoints)
        self.thresholds = ops.match_thresholds(thresholds)
        self.bins = int(bins)
        if self.num_keypoints < 1:
            raise ValueError("KeypointMetrics: need num_keypoints >= 1, got %d" % self.num_keypoints)
        if not 1 <= self.bins <= ops.PEAKS_MATCH_MAX_BINS:
            raise ValueError("KeypointMetrics: need 1 <= bins <= %d, got %d" % (ops.PEAKS_MATCH_MAX_BINS, self.bins))
        dev = torch.device("cpu") if device is None else torch.device(device)
        self._pinned = device is not None
        self.hist = torch.zeros((self.num_keypoints, len(self.thresholds), 2, self.bins), dtype=torch.int64,
                                device=dev)
        self.totals = torch.zeros((self.num_keypoints, 8), dtype=torch.int64, device=dev)

    @property
    def device(self):
        return self.hist.device

    def to(self, device):
        self.hist = self.hist.to(device)
        self.totals = self.totals.to(device)
        self._pinned = True
        return self

    def reset(self):
        self.hist.zero_()
        self.totals.zero_()

    def update(self, peaks, counts, labels, mask=None):
        """One launch, no synchronisation: peaks / counts as ops.heat_peaks returns
        them, labels [B,K,M,3] (u, v, flag) or [B,K,2], all on the accumulators'
        device.  mask uint8 [B,H,W] (hkp.masks, in the peaks' frame): the peaks on ignored
        pixels are dropped first (masks.peaks_drop_masked: they are neither true nor false
        positives, COCO's rule for ignore regions); still no synchronisation."""
        if not isinstance(peaks, torch.Tensor):
            raise HkpError("KeypointMetrics.update: expected tensors")
        if peaks.dim() == 4 and peaks.shape[1] != self.num_keypoints:
            raise HkpError("KeypointMetrics.update: peaks %s for %d keypoint classes"
                           % (tuple(peaks.shape), self.num_keypoints))
        if not self._pinned and self.hist.device != peaks.device and peaks.device.type == "cuda":
            self.to(peaks.device)
        if mask is not None:
            from .masks import peaks_drop_masked
            peaks, counts = peaks_drop_masked(peaks, counts, mask)
        ops.peaks_match(peaks, counts, labels, self.thresholds, self.hist, self.totals, bins=self.bins)

    def state(self):
        """(hist, totals) as int64 tensors on the CPU (one synchronising copy)."""
        return self.hist.cpu(), self.totals.cpu()

    def load_state(self, hist, totals):
        hist = torch.as_tensor(hist, dtype=torch.int64)
        totals = torch.as_tensor(totals, dtype=torch.int64)
        if hist.shape != self.hist.shape or totals.shape != self.totals.shape:
            raise ValueError("KeypointMetrics.load_state: need hist %s and totals %s, got %s and %s"
                             % (tuple(self.hist.shape), tuple(self.totals.shape), tuple(hist.shape),
                                tuple(totals.shape)))
        self.hist.copy_(hist)
        self.totals.copy_(totals)
        return self

    def merge(self, other):
        """Add another accumulator of the same classes, thresholds and bins."""
        if (other.num_keypoints, other.thresholds, other.bins) != (self.num_keypoints, self.thresholds, self.bins):
            raise ValueError("KeypointMetrics.merge: the two accumulators differ in classes, thresholds or bins")
        self.hist += other.hist.to(self.hist.device)
        self.totals += other.totals.to(self.totals.device)
        return self

    def all_reduce(self, group=None):
        """Sum of the accumulators over the ranks of `group`, on every rank: integer
        sums, so exact and independent of the rank order.  RCCL reduces int64 on the
        device; any other backend goes through host copies on a gloo group
        (parallel.host_group).  A no-op without torch.distributed."""
        import torch.distributed as dist
        if not dist.is_initialized() or dist.get_world_size(group) == 1:
            return self
        if self.hist.is_cuda and dist.get_backend(group) == "nccl":
            dist.all_reduce(self.hist, op=dist.ReduceOp.SUM, group=group)
            dist.all_reduce(self.totals, op=dist.ReduceOp.SUM, group=group)
            return self
        from .parallel import host_group
        hg = host_group(group)
        for t in (self.hist, self.totals):
            host = t.cpu().contiguous()
            dist.all_reduce(host, op=dist.ReduceOp.SUM, group=hg)
            t.copy_(host)
        return self

    def compute(self):
        """A plain dict (ints, floats, lists), in float64 from the integers alone:
        thresholds, bins; per_class[c]: planes, instances, peaks, absent_planes,
        absent_false_alarms, mean_error_px, and per threshold true_positives,
        false_positives, recall (PCK: TP / instances), precision, ap; overall: mAP
        (mean over the classes with instances and over the thresholds), recall and
        precision pooled over the classes, mean_error_px and the pooled counts.  A
        ratio with a zero denominator is nan."""
        hist, totals = self.state()
        return compute_from_state(hist.numpy(), totals.numpy(), self.thresholds)

    def summary(self):
        """One line: per-threshold pooled recall, mAP and mean error."""
        r = self.compute()["overall"]
        pck = " ".join("@%g %.4f" % (t, v) for t, v in zip(self.thresholds, r["recall"]))
        return "recall %s  mAP %.4f  mean error %.3f px" % (pck, r["mAP"], r["mean_error_px"])
