"""Keypoint evaluation without a GPU: the restatement of hkp_peaks_match
(tests/_metrics_ref.py; the kernel is held to it in test_gpu_metrics.py) pinned on
hand-written planes, KeypointMetrics.compute() on accumulators the restatement
fills, merge / all_reduce over a real 2-process gloo group, and the argument
checks that come before any library call."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import _metrics_ref as ref
from conftest import PKG, REPO

TH = (2.0, 4.0)


def _hand(name):
    for row in ref.hand_planes(4, 3):
        if row[0] == name:
            return row
    raise KeyError(name)


def _run_plane(name, bins=16):
    _, pk, cnt, lab, expect = _hand(name)
    out = ref.peaks_match(pk[None, None], np.array([[cnt]]), lab[None, None], TH, bins=bins)
    return out, expect


@pytest.mark.parametrize("name", [r[0] for r in ref.hand_planes(4, 3)])
def test_hand_planes_slots(name):
    (hist, totals, pm, gm, gd), expect = _run_plane(name)
    assert np.array_equal(pm[0, 0], expect["peak_match"]), pm[0, 0]
    assert np.array_equal(gm[0, 0], expect["gt_match"]), gm[0, 0]
    tp = (expect["peak_match"] >= 0).sum(axis=1)
    fp = (expect["peak_match"] == -1).sum(axis=1)
    assert np.array_equal(hist[0, :, 0].sum(axis=1), tp) and np.array_equal(hist[0, :, 1].sum(axis=1), fp)
    assert np.array_equal(gd[0, 0] >= 0, expect["gt_match"] >= 0)
    assert totals[0, 7] == 0


def test_hand_planes_counts():
    """The exact totals of the planes whose point is a count."""
    (_, tot, _, _, gd), _ = _run_plane("tie_instances")
    assert tot[0].tolist() == [1, 0, 2, 1, 1, 65536, 0, 0] and gd[0, 0].tolist() == [-1, 1, -1]
    (_, tot, _, _, _), _ = _run_plane("tie_peaks")
    assert tot[0].tolist() == [1, 0, 1, 2, 1, 65536, 0, 0]
    (_, tot, _, _, gd), _ = _run_plane("edge")              # 2 px and 2.25 px at the loosest threshold
    assert tot[0].tolist() == [1, 0, 2, 2, 2, 2 * 65536 + 9 * 65536 // 4, 0, 0]
    assert gd[0, 0].tolist() == [2.0, 2.25, -1.0]
    (hist, tot, _, _, _), _ = _run_plane("loose_only")
    assert tot[0].tolist() == [1, 0, 1, 1, 1, 3 * 65536, 0, 0]
    assert hist[0, 0, 1].sum() == 1 and hist[0, 0, 0].sum() == 0 and hist[0, 1, 0].sum() == 1
    (_, tot, _, _, _), _ = _run_plane("nan")
    assert tot[0].tolist() == [1, 0, 2, 2, 1, 65536, 0, 0]
    (hist, tot, _, _, _), _ = _run_plane("absent")
    assert tot[0].tolist() == [1, 1, 0, 2, 0, 0, 2, 0] and hist[0, :, 1].sum() == 4 and hist[0, :, 0].sum() == 0
    for name in ("cnt0", "cnt_neg"):
        (hist, tot, _, _, _), _ = _run_plane(name)
        assert tot[0].tolist() == [1, 0, 1, 0, 0, 0, 0, 0] and hist.sum() == 0
    (hist, tot, _, _, _), _ = _run_plane("cnt_big")         # P + 3 counts as P
    assert tot[0].tolist() == [1, 0, 1, 4, 1, 0, 0, 0] and hist[0, 1].sum() == 4


def test_unused_slots_are_never_read():
    """What lies in peak slots >= cnt and in the (u, v) of empty label slots does
    not reach any output."""
    pk, ct, lab = ref.hand_batch(2, 4, 3)
    want = ref.peaks_match(pk, ct, lab, TH, bins=8)
    pk2, lab2 = pk.copy(), lab.copy()
    for r in range(pk.shape[0]):
        for c in range(2):
            pk2[r, c, min(max(ct[r, c], 0), 4):] = (7.0, 7.0, 0.5)
    lab2[lab[..., 2] <= 0, :2] = 30.0
    got = ref.peaks_match(pk2, ct, lab2, TH, bins=8)
    for a, b in zip(want, got):
        assert np.array_equal(a, b)


def test_score_bins():
    bins = 1024
    assert ref.score_bin(0.0, bins) == 0
    assert ref.score_bin(-0.0, bins) == 0
    assert ref.score_bin(1.0, bins) == bins - 1
    assert ref.score_bin(1.5, bins) == bins - 1
    assert ref.score_bin(np.nan, bins) == 0
    assert ref.score_bin(-3.0, bins) == 0
    assert ref.score_bin(np.nextafter(np.float32(1), np.float32(0)), bins) == bins - 1
    for bn in (7, 1024, 4096):
        for b in range(bn):
            assert ref.score_bin(np.float32((b + 0.5) / bn), bn) == b, (bn, b)


def _centre_scores(pk, ct, bins, rng):
    """Scores replaced by bin centres (i + 0.5) / bins, descending by slot."""
    pk = pk.copy()
    for b in range(pk.shape[0]):
        for c in range(pk.shape[1]):
            n = min(max(int(ct[b, c]), 0), pk.shape[2])
            idx = np.sort(rng.integers(0, bins, n))[::-1]
            pk[b, c, :n, 2] = ((idx + 0.5) / bins).astype(np.float32)
    return pk


def test_compute_against_exact_ap():
    from hkp.metrics import KeypointMetrics
    B, K, P, M, bins = 6, 3, 8, 6, 64
    th = (2.0, 4.0, 8.0, 16.0)
    rng = np.random.default_rng(5)
    pk, ct, lab = ref.random_batch(11, B, K, P, M)
    lab[:, 2, :, 2] = 0                                   # class 2 never has an instance
    pk = _centre_scores(pk, ct, bins, rng)
    hist, totals, pm, gm, gd = ref.peaks_match(pk, ct, lab, th, bins=bins)
    res = KeypointMetrics(K, th, bins=bins).load_state(hist, totals).compute()
    assert res["thresholds"] == list(th) and res["bins"] == bins
    aps = []
    for c in range(K):
        r = res["per_class"][c]
        inst = int((lab[:, c, :, 2] > 0).sum())
        assert r["instances"] == inst == totals[c, 2] and r["peaks"] == int(ct[:, c].clip(0, P).sum())
        assert r["absent_planes"] == int(((lab[:, c, :, 2] > 0).sum(axis=1) == 0).sum())
        assert r["absent_false_alarms"] == totals[c, 6]
        for ti in range(len(th)):
            used = pm[:, c, ti] > -2
            tp = int((pm[:, c, ti] >= 0).sum())
            fp = int((pm[:, c, ti] == -1).sum())
            assert r["true_positives"][ti] == tp and r["false_positives"][ti] == fp
            want = ref.exact_ap(pk[:, c, :, 2][used], pm[:, c, ti][used] >= 0, inst)
            if inst:
                assert r["recall"][ti] == tp / inst and r["precision"][ti] == tp / (tp + fp)
                assert abs(r["ap"][ti] - want) < 1e-12, (c, ti, r["ap"][ti], want)
                assert 0.0 < r["ap"][ti] < 1.0
                aps.append(r["ap"][ti])
            else:
                assert np.isnan(r["ap"][ti]) and np.isnan(r["recall"][ti]) and np.isnan(want)
        if inst:
            matched = gd[:, c] >= 0
            assert r["mean_error_px"] == sum(ref.dist_q16(d) for d in gd[:, c][matched]) / 65536.0 / matched.sum()
            assert abs(r["mean_error_px"] - gd[:, c][matched].astype(np.float64).mean()) < 2.0 ** -16
        else:
            assert np.isnan(r["mean_error_px"])
    assert len(aps) == 2 * len(th)
    assert res["overall"]["mAP"] == float(np.mean(aps))
    for ti in range(len(th)):
        assert res["overall"]["recall"][ti] == (pm[:, :, ti] >= 0).sum() / (lab[..., 2] > 0).sum()
    assert res["overall"]["instances"] == int((lab[..., 2] > 0).sum())


def test_ap_known_values():
    from hkp.metrics import average_precision
    bins = 8
    tp, fp = np.zeros(bins, np.int64), np.zeros(bins, np.int64)
    assert average_precision(tp, fp, 4) == 0.0 and np.isnan(average_precision(tp, fp, 0))
    tp[7] = 4                                             # all found, nothing else
    assert average_precision(tp, fp, 4) == 1.0
    fp[0] = 9                                             # false positives below every true one
    assert average_precision(tp, fp, 4) == 1.0
    tp[:] = 0
    fp[:] = 0
    tp[7], fp[5], tp[3] = 1, 1, 1                         # recall 0.5 at precision 1, recall 1 at 2/3
    want = (51 * 1.0 + 50 * (2.0 / 3.0)) / 101
    assert abs(average_precision(tp, fp, 2) - want) < 1e-15
    tp[3] = 0                                             # recall stops at 0.5
    assert abs(average_precision(tp, fp, 2) - 51.0 / 101) < 1e-15


def test_merge_equals_whole_batch():
    from hkp.metrics import KeypointMetrics
    th = (2.0, 8.0)
    pk, ct, lab = ref.random_batch(3, 4, 2, 4, 3)
    whole = ref.peaks_match(pk, ct, lab, th, bins=32)
    a = KeypointMetrics(2, th, bins=32).load_state(*ref.peaks_match(pk[:1], ct[:1], lab[:1], th, bins=32)[:2])
    b = KeypointMetrics(2, th, bins=32).load_state(*ref.peaks_match(pk[1:], ct[1:], lab[1:], th, bins=32)[:2])
    a.merge(b)
    h, t = a.state()
    assert np.array_equal(h.numpy(), whole[0]) and np.array_equal(t.numpy(), whole[1])
    a.reset()
    assert int(a.state()[0].sum()) == 0 and int(a.state()[1].sum()) == 0
    with pytest.raises(ValueError):
        a.merge(KeypointMetrics(2, (2.0, 4.0), bins=32))
    with pytest.raises(ValueError):
        a.merge(KeypointMetrics(2, th, bins=16))
    assert a.all_reduce() is a                            # no process group: a no-op


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _reduce_worker(rank, world, port, q):
    import sys
    sys.path[:0] = [REPO, PKG, os.path.join(REPO, "tests")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import _metrics_ref as r
    from hkp import parallel
    from hkp.metrics import KeypointMetrics
    th = (2.0, 4.0, 16.0)
    pk, ct, lab = r.random_batch(17, 5, 3, 4, 3)
    whole = r.peaks_match(pk, ct, lab, th, bins=64)
    lo, hi = parallel.shard_range(5, rank, world)
    m = KeypointMetrics(3, th, bins=64).load_state(*r.peaks_match(pk[lo:hi], ct[lo:hi], lab[lo:hi], th, bins=64)[:2])
    m.all_reduce()
    h, t = m.state()
    q.put((rank, bool(np.array_equal(h.numpy(), whole[0])), bool(np.array_equal(t.numpy(), whole[1])),
           int(t[:, 0].sum())))
    dist.destroy_process_group()


def test_all_reduce_gloo_world2():
    """The halves of a batch on two ranks give exactly the integers of the whole."""
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_reduce_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
    res = [q.get(timeout=5) for _ in range(world)]
    assert all(p.exitcode == 0 for p in procs)
    assert all(a and b and planes == 15 for _, a, b, planes in res), res


def test_argument_validation(monkeypatch):
    """Bad arguments raise before any library call."""
    from hkp import _lib, ops
    from hkp.metrics import KeypointMetrics

    def no_call(*a, **k):
        raise AssertionError("library call")
    monkeypatch.setattr(ops, "call", no_call)
    monkeypatch.setattr(_lib, "lib", no_call)
    for bad in ((), (1,) * 9, (2.0, 2.0), (4.0, 2.0), (0.0, 1.0), (-1.0,), (float("nan"),), (1.0, float("inf")),
                (1e-46,), 3.0):
        with pytest.raises(ValueError):
            KeypointMetrics(2, bad)
    for bins in (0, 4097):
        with pytest.raises(ValueError):
            KeypointMetrics(2, bins=bins)
    with pytest.raises(ValueError):
        KeypointMetrics(0)
    m = KeypointMetrics(2, (2.0, 4.0), bins=8)
    assert m.thresholds == (2.0, 4.0) and tuple(m.hist.shape) == (2, 2, 2, 8) and tuple(m.totals.shape) == (2, 8)
    assert m.hist.dtype == torch.int64 and m.totals.dtype == torch.int64
    pk = torch.zeros((1, 2, 4, 3))
    ct = torch.zeros((1, 2), dtype=torch.int32)
    lab = torch.zeros((1, 2, 3, 3))
    with pytest.raises(_lib.HkpError, match="GPU"):       # no CPU path
        m.update(pk, ct, lab)
    with pytest.raises(_lib.HkpError, match="classes"):
        m.update(torch.zeros((1, 3, 4, 3)), ct, lab)
    with pytest.raises(_lib.HkpError):
        m.update(None, ct, lab)
    with pytest.raises(ValueError):
        ops.peaks_match(pk, ct, lab, (2.0,), m.hist, m.totals, bins=0)
    with pytest.raises(ValueError):
        m.load_state(np.zeros((2, 2, 2, 4)), np.zeros((2, 8)))
