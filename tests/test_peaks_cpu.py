"""The multi-peak decode's definition, pinned on its numpy restatement
(tests/_peaks_ref.py; the kernel hkp_heat_peaks is held to it in
tests/test_gpu_peaks.py), and hkp.parallel.gather_peaks over a gloo group.  No GPU."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import _peaks_ref as ref
from conftest import PKG, REPO

h, w, H, W = 60, 80, 480, 640


def ideal_logits(cx, cy, sigma, hw=(h, w), HW=(H, W)):
    """fp32 logits of p = exp(-d^2 / 2 sigma^2) sampled at the align_corners nodes."""
    ys = np.arange(hw[0], dtype=np.float64) * (HW[0] - 1) / (hw[0] - 1)
    xs = np.arange(hw[1], dtype=np.float64) * (HW[1] - 1) / (hw[1] - 1)
    d2 = (ys[:, None] - cy) ** 2 + (xs[None, :] - cx) ** 2
    p = np.clip(np.exp(-d2 / (2.0 * sigma * sigma)), 1e-30, 1.0 - 2.0 ** -24)
    return (np.log(p) - np.log1p(-p)).astype(np.float32)


@pytest.mark.parametrize("sigma", [4, 8])
def test_ideal_gaussian_is_recovered_below_the_lattice(sigma):
    rng = np.random.default_rng(sigma)
    refined, lattice = [], []
    for _ in range(40):
        cx, cy = rng.uniform(40, W - 1 - 40), rng.uniform(40, H - 1 - 40)
        z = ideal_logits(cx, cy, sigma)
        picked = []
        peaks, count = ref.plane_peaks(z, H, W, max_peaks=1, radius=1, picked=picked)
        assert count == 1
        refined.append(np.hypot(float(peaks[0, 0]) - cx, float(peaks[0, 1]) - cy))
        # the full-resolution pixel nearest to the node: what an argmax of the upsampled map can give
        i, j = picked[0]
        lattice.append(np.hypot(np.rint(j * (W - 1) / (w - 1)) - cx, np.rint(i * (H - 1) / (h - 1)) - cy))
    print("sigma %d: refined max %.3g px, lattice mean %.3g px max %.3g px"
          % (sigma, max(refined), np.mean(lattice), max(lattice)))
    assert max(refined) < 1e-4
    assert np.mean(lattice) > 2.0


def _random_plane(rng, hh, ww):
    return np.clip(np.round(rng.normal(0, 3, (hh, ww)) * 8) / 8, -10, 10).astype(np.float32)


@pytest.mark.parametrize("r", [1, 2, 8])
def test_no_two_peaks_within_the_radius(r):
    rng = np.random.default_rng(10 + r)
    for hh, ww in ((7, 9), (31, 45), (1, 40), (40, 1)):
        z = _random_plane(rng, hh, ww)                     # quantised: ties
        picked = []
        _, count = ref.plane_peaks(z, 8 * hh, 8 * ww, max_peaks=16, radius=r, picked=picked)
        assert count == len(picked) >= 1
        for a in range(count):
            for b in range(a + 1, count):
                assert max(abs(picked[a][0] - picked[b][0]), abs(picked[a][1] - picked[b][1])) > r
        # every candidate, not only the 16 written
        cand = np.argwhere(ref.window_maxima(ref.canonical(z), r))
        d = np.abs(cand[:, None, :] - cand[None, :, :]).max(-1)
        assert (d[~np.eye(len(cand), dtype=bool)] > r).all()


def test_order_threshold_counts_and_unused_slots():
    z = np.full((9, 12), -6.0, dtype=np.float32)
    for (i, j), v in {(1, 1): 2.0, (1, 6): 3.0, (5, 3): 2.0, (7, 10): -1.0, (4, 8): 0.0}.items():
        z[i, j] = v
    picked = []
    peaks, count = ref.plane_peaks(z, 72, 96, max_peaks=8, radius=1, picked=picked)
    # by value, ties by index; the -6 background yields none: each of its nodes has an equal
    # earlier neighbour, except (0, 0), which (1, 1) beats
    assert count == 5
    assert picked[:5] == [(1, 6), (1, 1), (5, 3), (4, 8), (7, 10)]
    assert (np.diff(peaks[:count, 2]) <= 0).all()
    assert np.array_equal(peaks[count:], np.tile(np.float32([-1, -1, 0]), (8 - count, 1)))
    s = ref.sigmoid_f32(np.float32([3.0, 2.0, 0.0, -1.0]))
    assert peaks[0, 2] == s[0] and peaks[1, 2] == s[1] and peaks[2, 2] == s[1] and peaks[3, 2] == s[2]
    # threshold keeps score >= t (equality included)
    for t, want in ((0.0, count), (float(s[2]), 4), (0.51, 3), (float(s[0]), 1), (0.99, 0)):
        pk, c = ref.plane_peaks(z, 72, 96, max_peaks=8, radius=1, threshold=t)
        assert c == want, (t, c)
        assert np.array_equal(pk[:c], peaks[:c])
        assert np.array_equal(pk[c:], np.tile(np.float32([-1, -1, 0]), (8 - c, 1)))
    # max_peaks cuts the same list short
    pk, c = ref.plane_peaks(z, 72, 96, max_peaks=2, radius=1)
    assert c == 2 and np.array_equal(pk, peaks[:2])
    # batched form
    low = np.stack([z, -z])[None]
    pk, ct = ref.heat_peaks(low, 72, 96, max_peaks=8, radius=1)
    assert pk.shape == (1, 2, 8, 3) and pk.dtype == np.float32 and ct.shape == (1, 2) and ct.dtype == np.int32
    assert np.array_equal(pk[0, 0], peaks) and ct[0, 0] == count


@pytest.mark.parametrize("r", [1, 2])
def test_plateau_gives_one_peak_at_its_first_index(r):
    z = np.full((12, 14), -3.0, dtype=np.float32)
    z[4:4 + r + 1, 5:5 + r + 1] = 1.5                       # (r+1)^2 equal nodes: inside one window
    picked = []
    peaks, count = ref.plane_peaks(z, 96, 112, max_peaks=16, radius=r, picked=picked)
    assert picked[0] == (4, 5)
    assert sum(1 for p in picked if z[p] == np.float32(1.5)) == 1


def test_nan_and_infinite_nodes():
    z = np.full((6, 7), -np.inf, dtype=np.float32)
    peaks, count = ref.plane_peaks(z, 48, 56, max_peaks=4)
    assert count == 0 and np.array_equal(peaks, np.tile(np.float32([-1, -1, 0]), (4, 1)))
    z[:] = np.nan                                          # NaN counts as -inf
    assert ref.plane_peaks(z, 48, 56, max_peaks=4)[1] == 0
    for c in (0.0, -0.0, 2.5, np.inf):                     # a constant plane: one peak, at index 0
        z[:] = c
        picked = []
        peaks, count = ref.plane_peaks(z, 48, 56, max_peaks=4, radius=8, picked=picked)
        assert count == 1 and picked == [(0, 0)] and tuple(peaks[0, :2]) == (0.0, 0.0)
    z = np.zeros((6, 7), dtype=np.float32)
    z[0, 3] = -0.0                                         # -0 == +0: the earlier index still wins
    assert ref.plane_peaks(z, 48, 56, max_peaks=4, radius=8)[1] == 1
    z = np.full((6, 7), -2.0, dtype=np.float32)
    z[2, 2], z[2, 3], z[4, 5], z[3, 5] = np.inf, np.nan, 1.0, -np.inf
    picked = []
    peaks, count = ref.plane_peaks(z, 48, 56, max_peaks=4, picked=picked)
    assert picked[:2] == [(2, 2), (4, 5)]
    assert peaks[0, 2] == 1.0                              # sigmoid(+inf)
    # (2, 2): its right neighbour is NaN -> g = -inf -> no x offset; up and down are finite
    assert peaks[0, 0] == np.float32(2 * 55 / 6) and np.isfinite(peaks[0, 1])
    # (4, 5): the node above is -inf -> no y offset
    assert peaks[1, 1] == np.float32(4 * 47 / 5)


def test_border_nodes_and_single_row_planes_have_no_offset():
    rng = np.random.default_rng(3)
    z = rng.normal(0, 1, (5, 6)).astype(np.float32)
    z[0, 0], z[4, 3], z[2, 5] = 9.0, 8.0, 7.0
    peaks, count = ref.plane_peaks(z, 40, 48, max_peaks=3)
    assert count == 3
    assert tuple(peaks[0, :2]) == (0.0, 0.0)                                   # corner: neither axis
    assert peaks[1, 1] == np.float32(39.0) and peaks[1, 0] != np.float32(3 * 47 / 5)   # bottom row: x only
    assert peaks[2, 0] == np.float32(47.0) and peaks[2, 1] != np.float32(2 * 39 / 4)   # right column: y only
    row = np.float32([[0, 1, 3, 2.5, 0, 0, 0, 4]])
    peaks, count = ref.plane_peaks(row, 1, 64, max_peaks=4)
    assert count == 2 and (peaks[:2, 1] == 0).all()                            # h == 1: y = 0
    assert peaks[0, 0] == np.float32(63.0) and 2 * 9 < peaks[1, 0] < 2.5 * 9   # pulled towards the 2.5
    peaks, count = ref.plane_peaks(row.T, 64, 1, max_peaks=4)
    assert count == 2 and (peaks[:2, 0] == 0).all() and peaks[0, 1] == np.float32(63.0)
    peaks, count = ref.plane_peaks(np.float32([[0.25]]), 8, 8, max_peaks=2)
    assert count == 1 and tuple(peaks[0, :2]) == (0.0, 0.0)


def test_invert_peaks_maps_only_the_used_slots():
    from hkp import resample
    plan = resample.Resize("bilinear", mode="fit").plan([(150, 330), (64, 96)], (64, 96))
    rng = np.random.default_rng(5)
    peaks = rng.uniform(0, 60, (2, 3, 4, 3)).astype(np.float32)
    counts = np.array([[4, 2, 0], [1, 3, 4]], dtype=np.int32)
    for n in range(2):
        for k in range(3):
            peaks[n, k, counts[n, k]:] = (-1, -1, 0)
    got = plan.invert_peaks(peaks, counts)
    want = plan.invert_uv(peaks[..., :2].reshape(2, 12, 2)).reshape(2, 3, 4, 2)
    for n in range(2):
        for k in range(3):
            c = counts[n, k]
            assert np.array_equal(got[n, k, :c, :2], want[n, k, :c])
            assert np.array_equal(got[n, k, c:], peaks[n, k, c:])
    assert np.array_equal(got[..., 2], peaks[..., 2])
    assert np.array_equal(got[1], peaks[1])                 # an image of the output's size maps to itself
    t = plan.invert_peaks(torch.from_numpy(peaks), torch.from_numpy(counts))
    assert isinstance(t, torch.Tensor) and np.array_equal(t.numpy(), got)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gather_worker(rank, world, port, q):
    import sys
    sys.path[:0] = [REPO, PKG]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from hkp import parallel
    n, K, P = 5, 3, 4                                       # shards of 3 and 2 images
    lo, hi = parallel.shard_range(n, rank, world)
    allp = torch.arange(n * K * P * 3, dtype=torch.float32).reshape(n, K, P, 3) / 7
    allc = (torch.arange(n * K, dtype=torch.int32).reshape(n, K) % (P + 1)).to(torch.int32)
    gp, gc = parallel.gather_peaks(allp[lo:hi].clone(), allc[lo:hi].clone())
    bad = 0
    for args in ((allp[lo:hi].double(), allc[lo:hi]), (allp[lo:hi], allc[lo:hi].long()), (allp[lo:hi, :, :, :2], allc[lo:hi])):
        try:
            parallel.gather_peaks(*args)
        except ValueError:
            bad += 1
    q.put((rank, hi - lo, torch.equal(gp, allp) and gp.dtype == torch.float32,
           torch.equal(gc, allc) and gc.dtype == torch.int32, bad))
    dist.destroy_process_group()


def test_gather_peaks_gloo_world2_unequal_shards():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gather_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
    res = sorted(q.get(timeout=5) for _ in range(world))
    assert all(p.exitcode == 0 for p in procs)
    assert [r[1] for r in res] == [3, 2]
    assert all(okp and okc and bad == 3 for _, _, okp, okc, bad in res), res


def test_gather_peaks_single_process_passthrough():
    from hkp import parallel
    p, c = torch.zeros(2, 3, 4, 3), torch.zeros(2, 3, dtype=torch.int32)
    gp, gc = parallel.gather_peaks(p, c)
    assert gp is p and gc is c
