"""numpy restatement of hkp_peaks_match (include/hulkkp.h): the decoded peaks of
hkp_heat_peaks matched to the instance labels, by its definition, with plain loops
in float64.

Per plane (b, c) of peaks [n][k][p][3] (x, y, score), counts [n][k], pts [n][k][m][3]
(u, v, flag) and thresholds tau[0..t) (fp32, ascending):
  slots      cnt = clamp(counts, 0, p); peak slots >= cnt are never read; a label slot
             is present iff flag > 0 and the (u, v) of an empty slot are never read.
  distance   dx = (double)x - (double)u, dy likewise, d2 = dx*dx + dy*dy; within tau
             means d2 <= (double)tau * (double)tau, so NaN never matches.
  matching   per threshold, the peaks in slot order each take the nearest present,
             not yet taken instance within tau; equal d2: the lower label slot.
  score bin  fp32: s >= 1 -> bins-1; not (s > 0) -> 0; else min(bins-1, int(s * bins)).
  hist       [k][t][2][bins] += 1 at [c][ti][0 = TP, 1 = FP][bin].
  totals     [k][8]: planes, absent planes, present instances, peaks, instances matched
             at the loosest threshold, sum of floor(dist32 * 65536 + 0.5) over those,
             peaks on absent planes, untouched.
  outputs    peak_match [n][k][t][p] (slot, -1 unmatched, -2 unused), gt_match
             [n][k][m] (peak slot, -1 missed, -2 empty), gt_dist [n][k][m] fp32 (-1).
"""
import numpy as np


def score_bin(s, bins):
    s = np.float32(s)
    if s >= np.float32(1):
        return bins - 1
    if not s > np.float32(0):
        return 0
    return min(bins - 1, int(np.float32(s * np.float32(bins))))


def dist_q16(dist32):
    return int(np.floor(np.float64(np.float32(dist32)) * 65536.0 + 0.5))


def peaks_match(peaks, counts, pts, thresholds, bins=1024, hist=None, totals=None):
    """Returns (hist, totals, peak_match, gt_match, gt_dist); hist / totals given are
    added to in place."""
    peaks = np.asarray(peaks, dtype=np.float32)
    counts = np.asarray(counts)
    pts = np.asarray(pts, dtype=np.float32)
    if pts.ndim == 3:                      # [n, k, 2]: one present instance per plane
        pts = np.concatenate([pts, np.ones_like(pts[..., :1])], axis=2)[:, :, None, :]
    n, k, p, _ = peaks.shape
    m = pts.shape[2]
    th = [np.float32(v) for v in thresholds]
    t = len(th)
    if hist is None:
        hist = np.zeros((k, t, 2, bins), dtype=np.int64)
    if totals is None:
        totals = np.zeros((k, 8), dtype=np.int64)
    peak_match = np.full((n, k, t, p), -2, dtype=np.int32)
    gt_match = np.full((n, k, m), -2, dtype=np.int32)
    gt_dist = np.full((n, k, m), -1, dtype=np.float32)
    for b in range(n):
        for c in range(k):
            cnt = min(max(int(counts[b, c]), 0), p)
            present = [i for i in range(m) if pts[b, c, i, 2] > 0]
            totals[c, 0] += 1
            totals[c, 1] += 0 if present else 1
            totals[c, 2] += len(present)
            totals[c, 3] += cnt
            totals[c, 6] += 0 if present else cnt
            d2 = {}
            for j in range(cnt):
                for i in present:
                    dx = np.float64(peaks[b, c, j, 0]) - np.float64(pts[b, c, i, 0])
                    dy = np.float64(peaks[b, c, j, 1]) - np.float64(pts[b, c, i, 1])
                    with np.errstate(invalid="ignore", over="ignore"):
                        d2[j, i] = dx * dx + dy * dy
            for ti in range(t):
                tau2 = np.float64(th[ti]) * np.float64(th[ti])
                taken = {}
                for j in range(cnt):
                    best = -1
                    for i in present:
                        if i in taken or not d2[j, i] <= tau2:
                            continue
                        if best < 0 or d2[j, i] < d2[j, best]:
                            best = i
                    peak_match[b, c, ti, j] = best
                    if best >= 0:
                        taken[best] = j
                    hist[c, ti, 0 if best >= 0 else 1, score_bin(peaks[b, c, j, 2], bins)] += 1
                if ti == t - 1:
                    for i in present:
                        gt_match[b, c, i] = taken.get(i, -1)
                        if i in taken:
                            d = np.float32(np.sqrt(d2[taken[i], i]))
                            gt_dist[b, c, i] = d
                            totals[c, 4] += 1
                            totals[c, 5] += dist_q16(d)
    return hist, totals, peak_match, gt_match, gt_dist


# ---- inputs shared by the CPU and GPU tests -----------------------------------

def hand_planes(P=4, M=3):
    """Hand-written planes with known answers, thresholds (2, 4): a list of
    (name, peaks [P,3], count, pts [M,3], expect) with expect = dict of
    peak_match [2][P], gt_match [M].  Unused peak slots hold NaN / 1e30, empty label
    slots NaN."""
    nan = np.nan
    out = []

    def plane(name, pk, cnt, lab, pm, gm):
        peaks = np.full((P, 3), nan, dtype=np.float32)
        peaks[:, 1] = 1e30
        for j, row in enumerate(pk):
            peaks[j] = row
        pts = np.full((M, 3), nan, dtype=np.float32)
        pts[:, 2] = 0
        for i, row in enumerate(lab):
            if row is not None:
                pts[i] = row
        full = np.full((2, P), -2, dtype=np.int32)
        for ti in range(2):
            full[ti, :len(pm[ti])] = pm[ti]
        out.append((name, peaks, cnt, pts, {"peak_match": full, "gt_match": np.array(gm, dtype=np.int32)}))

    # two instances equidistant from one peak: the lower slot wins
    plane("tie_instances", [(10, 10, .9)], 1, [None, (11, 10, 1), (9, 10, 1)], [[1], [1]], [-2, 0, -1])
    # two peaks equidistant from one instance: the earlier peak wins, the later is a false positive
    plane("tie_peaks", [(21, 20, .9), (19, 20, .8)], 2, [(20, 20, 1)], [[0, -1], [0, -1]], [0, -2, -2])
    # exactly on the threshold matches, a quarter pixel beyond does not (tau = 2, then 4)
    plane("edge", [(32, 30, .9), (44.25, 40, .8)], 2, [(30, 30, 1), (42, 40, 1)], [[0, -1], [0, 1]], [0, 1, -2])
    plane("edge4", [(54, 50, .9), (64.25, 60, .8)], 2, [(50, 50, 1), (60, 60, 1)], [[-1, -1], [0, -1]], [0, -1, -2])
    # a match at the loose threshold that is a false positive at the tight one
    plane("loose_only", [(73, 70, .7)], 1, [(70, 70, 1)], [[-1], [0]], [0, -2, -2])
    # peak 1 is nearer to the instance peak 0 took: it falls through to the second nearest
    plane("fall_through", [(80, 80, .9), (80.5, 80, .8)], 2, [(80, 80, 1), (82, 80, 1)], [[0, 1], [0, 1]],
          [0, 1, -2])
    # NaN instance: a miss; NaN peak: a false positive
    plane("nan", [(nan, 90, .9), (90, 90, .8)], 2, [(nan, nan, 1), (90, 91, 1)], [[-1, 1], [-1, 1]], [-1, 1, -2])
    # an absent plane with peaks
    plane("absent", [(5, 5, .9), (50, 5, .3)], 2, [], [[-1, -1], [-1, -1]], [-2, -2, -2])
    # counts of 0, -1 and P + 3
    plane("cnt0", [(30, 30, .9)], 0, [(30, 30, 1)], [[], []], [-1, -2, -2])
    plane("cnt_neg", [(30, 30, .9)], -1, [(30, 30, 1)], [[], []], [-1, -2, -2])
    plane("cnt_big", [(30, 30, .9), (0, 0, .5), (0, 1, .4), (0, 2, .3)], P + 3, [(30, 30, 1)],
          [[0, -1, -1, -1], [0, -1, -1, -1]], [0, -2, -2])
    return out


def hand_batch(K, P, M):
    """The hand planes as batch rows: every row holds plane r in each class (cut to
    the first P peak slots and M label slots where those are fewer than 4 and 3).
    Returns (peaks [R,K,P,3], counts [R,K], pts [R,K,M,3])."""
    rows = hand_planes(4, 3)
    R = len(rows)
    peaks = np.full((R, K, P, 3), np.nan, dtype=np.float32)
    peaks[..., 1] = 1e30
    counts = np.zeros((R, K), dtype=np.int32)
    pts = np.full((R, K, M, 3), np.nan, dtype=np.float32)
    pts[..., 2] = 0
    for r, (_, pk, cnt, lab, _) in enumerate(rows):
        peaks[r, :, :min(P, 4)] = pk[:min(P, 4)]
        counts[r, :] = cnt if cnt <= 4 else P + 3
        pts[r, :, :min(M, 3)] = lab[:min(M, 3)]
    return peaks, counts, pts


DISTANCES = (0, 1, 2, 3, 5, 8, 12, 20)


def random_batch(seed, B, K, P, M, size=200.0):
    """Seeded planes: 0-5 instances (at most M) in random slots at quarter-pixel
    coordinates, empty slots NaN; per instance with probability 0.8 a peak at a
    distance from DISTANCES along a multiple of 45 degrees, sometimes a second one
    4 px to its side; 0-3 stray peaks; at most P peaks, scores descending by slot;
    every fourth plane absent; unused peak slots NaN and 1e30."""
    rng = np.random.default_rng(seed)
    peaks = np.full((B, K, P, 3), np.nan, dtype=np.float32)
    peaks[..., 1] = 1e30
    counts = np.zeros((B, K), dtype=np.int32)
    pts = np.full((B, K, M, 3), np.nan, dtype=np.float32)
    pts[..., 2] = 0
    for b in range(B):
        for c in range(K):
            absent = (b * K + c) % 4 == 3
            ninst = 0 if absent else int(rng.integers(0, min(5, M) + 1))
            slots = sorted(rng.choice(M, size=ninst, replace=False).tolist())
            cand = []
            for i in slots:
                u, v = np.round(rng.uniform(20, size - 20, 2) * 4) / 4
                pts[b, c, i] = (u, v, 1)
                if rng.random() < 0.8:
                    d = DISTANCES[int(rng.integers(len(DISTANCES)))]
                    a = int(rng.integers(8)) * np.pi / 4
                    x, y = u + d * np.round(np.cos(a) * 1e6) / 1e6, v + d * np.round(np.sin(a) * 1e6) / 1e6
                    cand.append((x, y))
                    if rng.random() < 0.3:
                        cand.append((x + 4 * np.sin(a), y - 4 * np.cos(a)))
            for _ in range(int(rng.integers(0, 4))):
                cand.append(tuple(np.round(rng.uniform(0, size, 2) * 4) / 4))
            order = rng.permutation(len(cand))[:P]
            scores = np.sort(rng.uniform(0.02, 0.999, len(order)).astype(np.float32))[::-1]
            for j, q in enumerate(order):
                peaks[b, c, j] = (cand[q][0], cand[q][1], scores[j])
            counts[b, c] = len(order)
    return peaks, counts, pts


def exact_ap(scores, is_tp, instances, recall_points=None):
    """Sort-based AP: detections sorted by score descending, equal scores one step,
    precision monotone from the right, mean precision at the 101 recalls 0 .. 1."""
    if recall_points is None:
        recall_points = np.linspace(0.0, 1.0, 101)
    if instances <= 0:
        return float("nan")
    scores = np.asarray(scores, dtype=np.float64)
    is_tp = np.asarray(is_tp, dtype=bool)
    rec, prec = [], []
    tp = fp = 0
    for s in sorted(set(scores.tolist()), reverse=True):
        sel = scores == s
        tp += int(is_tp[sel].sum())
        fp += int((~is_tp[sel]).sum())
        rec.append(tp / float(instances))
        prec.append(tp / float(tp + fp))
    for i in range(len(prec) - 2, -1, -1):
        prec[i] = max(prec[i], prec[i + 1])
    q = []
    for r in recall_points:
        v = 0.0
        for rr, pp in zip(rec, prec):
            if rr >= r:
                v = pp
                break
        q.append(v)
    return float(np.mean(np.array(q, dtype=np.float64)))
