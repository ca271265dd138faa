"""Associative-embedding tags: which decoded keypoints belong to one cable
(not in the reference; Newell et al., 2017).

The tag map of class c is row K + c of the scoring conv (net.keypoints_forward(tags=True)
returns low_all [B,2K,h,w]); ops.tag_loss trains the tags of one label group together and
those of different groups apart, ops.peaks_group groups the peaks of ops.heat_peaks by tag.
This module holds what goes around the two kernels:

  slot_groups  the default group labels of instance labels pts [B,K,M,3]: slot m of every
               listed class is cable m (CableScenes.label_points, KeypointsDataset(instances=M)
               and the geometric augmentation keep slots in place), built once per shape and
               device and cached.
  pair_scores  host numpy: how well predicted groups agree with the label groups, from
               ops.peaks_match(outputs=True)'s gt_match.
"""
import numpy as np
import torch

_slot_cache = {}


def slot_groups(B, K, M, classes, device):
    """int32 [B,K,M] on `device`: gid = m in the rows of `classes` (class indices), -1
    elsewhere — the gid of ops.tag_loss when slot m of every listed class is instance m.
    Cached: the same arguments return the same tensor (do not write to it)."""
    B, K, M = int(B), int(K), int(M)
    cl = tuple(classes)
    for c in cl:
        if isinstance(c, bool) or not isinstance(c, int) or not 0 <= c < K:
            raise ValueError("slot_groups: classes %r: %r is no class index of 0..%d" % (cl, c, K - 1))
    if len(set(cl)) != len(cl) or not cl:
        raise ValueError("slot_groups: classes %r must name at least one class, none twice" % (cl,))
    if B < 1 or K < 1 or not 1 <= M <= 16:
        raise ValueError("slot_groups: need B, K >= 1 and 1 <= M <= 16, got %d, %d, %d" % (B, K, M))
    device = torch.device(device)
    key = (B, K, M, cl, device)
    g = _slot_cache.get(key)
    if g is None:
        host = np.full((B, K, M), -1, np.int32)
        host[:, list(cl), :] = np.arange(M, dtype=np.int32)
        g = _slot_cache[key] = torch.from_numpy(host).to(device)
    return g


def pair_scores(group, gt_match, gid):
    """group int [B,K,P] (ops.peaks_group), gt_match int [B,K,M] (ops.peaks_match(outputs=True):
    the peak slot that took label slot i at the loosest threshold, negative for none) and the
    label groups gid int [B,K,M] (negative or >= 32: the slot is in no group), as arrays on the
    host (tensors are copied) → dict:
      label_groups  the label groups with at least two matched members (per image)
      paired        the share of those whose matched peaks all carry ONE predicted group id
      pred_groups   the predicted groups that hold at least one matched peak
      mixed         the share of those whose matched peaks come from two or more label groups
    (shares of an empty set are 0.0).  Two caps paired with two tails at random give
    paired = 0.5."""
    group, gt_match, gid = (np.asarray(t.cpu() if isinstance(t, torch.Tensor) else t) for t in (group, gt_match, gid))
    B, K, M = gid.shape
    if gt_match.shape != gid.shape or group.shape[:2] != (B, K):
        raise ValueError("pair_scores: group %s, gt_match %s and gid %s do not go together"
                         % (group.shape, gt_match.shape, gid.shape))
    P = group.shape[2]
    n_label = n_paired = n_pred = n_mixed = 0
    for b in range(B):
        by_label, by_pred = {}, {}
        for c in range(K):
            for i in range(M):
                lg, j = int(gid[b, c, i]), int(gt_match[b, c, i])
                if not 0 <= lg < 32 or not 0 <= j < P:
                    continue
                pg = int(group[b, c, j])
                by_label.setdefault(lg, []).append(pg)
                if pg >= 0:
                    by_pred.setdefault(pg, set()).add(lg)
        for pgs in by_label.values():
            if len(pgs) >= 2:
                n_label += 1
                n_paired += int(pgs[0] >= 0 and all(v == pgs[0] for v in pgs))
        n_pred += len(by_pred)
        n_mixed += sum(1 for lgs in by_pred.values() if len(lgs) >= 2)
    return dict(label_groups=n_label, paired=n_paired / n_label if n_label else 0.0,
                pred_groups=n_pred, mixed=n_mixed / n_pred if n_pred else 0.0)
