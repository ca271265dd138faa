"""Associative-embedding tags without a GPU: the numpy restatement
(tests/_tags_ref.py; the kernels hkp_tag_loss and hkp_peaks_group are held to it in
tests/test_gpu_tags.py) against torch float64 autograd and central differences, its
grouping on hand cases, hkp.grouping's host helpers, and every rejection of the ops
wrappers and of the two C entries before anything is touched."""
import ctypes

import numpy as np
import pytest
import torch

import _tags_ref as ref


def _case(seed, B=2, K=3, M=4, h=5, w=7, H=33, W=49):
    rng = np.random.default_rng(seed)
    tags = rng.normal(0, 1, (B, K, h, w)).astype(np.float32)
    pts = np.zeros((B, K, M, 3), np.float32)
    pts[..., 0] = rng.uniform(0, W - 1, (B, K, M))
    pts[..., 1] = rng.uniform(0, H - 1, (B, K, M))
    pts[..., 2] = rng.random((B, K, M)) < 0.8
    gid = rng.integers(0, 3, (B, K, M)).astype(np.int32)
    return tags, pts, gid, H, W


def _torch_total(tags64, pts, gid, H, W, pull, push):
    """The same loss in torch float64 from the restatement's taps: autograd gives d total / d tags."""
    B, K, h, w = tags64.shape
    total = tags64.new_zeros(())
    for b in range(B):
        ts, gs = [], []
        for c in range(K):
            for m in range(pts.shape[2]):
                if pts[b, c, m, 2] > 0 and 0 <= gid[b, c, m] < 32:
                    _, taps = ref.sample(np.zeros((h, w), np.float32), pts[b, c, m, 0], pts[b, c, m, 1], H, W)
                    (y0, x0, _), (_, x1, _), (y1, _, _), _ = taps
                    fx = taps[1][2] + taps[3][2]
                    fy = taps[2][2] + taps[3][2]
                    p = tags64[b, c]
                    top = (1 - fx) * p[y0, x0] + fx * p[y0, x1]
                    bot = (1 - fx) * p[y1, x0] + fx * p[y1, x1]
                    ts.append((1 - fy) * top + fy * bot)
                    gs.append(int(gid[b, c, m]))
        ids = sorted(set(gs))
        if not ids:
            continue
        mu = {q: sum(t for t, g in zip(ts, gs) if g == q) / gs.count(q) for q in ids}
        pl = sum(sum((t - mu[q]) ** 2 for t, g in zip(ts, gs) if g == q) / gs.count(q) for q in ids) / len(ids)
        ps = tags64.new_zeros(())
        if len(ids) >= 2:
            ps = sum(torch.exp(-(mu[a] - mu[b2]) ** 2 / 2) for a in ids for b2 in ids if a != b2) \
                / (len(ids) * (len(ids) - 1))
        total = total + pull * pl + push * ps
    return total / B


@pytest.mark.parametrize("pull,push", [(1.0, 1.0), (0.5, 2.0), (1.0, 0.0), (0.0, 1.0)])
def test_closed_form_gradient_against_autograd_and_differences(pull, push):
    tags, pts, gid, H, W = _case(3)
    out, dtag = ref.tag_loss(tags, pts, gid, H, W, scale=1.0, pull=pull, push=push)
    t64 = torch.from_numpy(tags.astype(np.float64)).requires_grad_(True)
    total = _torch_total(t64, pts, gid, H, W, pull, push)
    total.backward()
    assert abs(out[0] - total.item()) <= 1e-13 * max(1.0, abs(total.item()))
    np.testing.assert_allclose(dtag, t64.grad.numpy(), rtol=1e-11, atol=1e-14)
    assert abs(out[0] - (pull * out[1] + push * out[2])) <= 1e-14
    # central differences of the restatement's own total at a few nodes that carry gradient
    nz = np.argwhere(np.abs(dtag) > 1e-6)[:6]
    assert len(nz)
    for idx in nz:
        idx = tuple(idx)
        eps = 2.0 ** -10                      # exact in fp32 next to values of order 1
        tp, tm = tags.copy(), tags.copy()
        tp[idx] += eps
        tm[idx] -= eps
        step = float(tp[idx]) - float(tm[idx])
        num = (ref.tag_loss(tp, pts, gid, H, W, 1.0, pull, push)[0][0]
               - ref.tag_loss(tm, pts, gid, H, W, 1.0, pull, push)[0][0]) / step
        assert abs(num - dtag[idx]) <= 1e-5 * max(1.0, abs(dtag[idx])), (idx, num, dtag[idx])


def test_scale_is_linear_and_out_does_not_depend_on_it():
    tags, pts, gid, H, W = _case(4)
    o1, d1 = ref.tag_loss(tags, pts, gid, H, W, scale=1.0)
    o2, d2 = ref.tag_loss(tags, pts, gid, H, W, scale=0.25)
    assert np.array_equal(o1, o2)
    np.testing.assert_allclose(d2, 0.25 * d1, rtol=1e-15, atol=0)


def test_zero_when_groups_coincide_and_push_is_off():
    B, K, M, h, w, H, W = 1, 2, 3, 4, 5, 25, 33
    tags = np.zeros((B, K, h, w), np.float32)
    tags[0, 0], tags[0, 1] = 0.75, 0.75           # constant maps: every sample is the constant
    pts = np.zeros((B, K, M, 3), np.float32)
    pts[..., 0], pts[..., 1], pts[..., 2] = 7.3, 11.9, 1
    gid = np.tile(np.arange(M, dtype=np.int32), (B, K, 1))
    out, dtag = ref.tag_loss(tags, pts, gid, H, W, 1.0, pull=1.0, push=0.0)
    assert out[0] == 0.0 and out[1] == 0.0 and not dtag.any()
    assert out[2] == 1.0                          # all means equal: every pair pushes with exp(0)


def test_push_alone_is_symmetric_in_the_two_groups():
    t = np.array([0.3, -1.1, 0.9, 0.2])
    g = np.array([0, 0, 5, 5])
    _, ps, _, dps = ref.image_loss(t, g)
    _, ps2, _, dps2 = ref.image_loss(t[[2, 3, 0, 1]], g)          # the groups' tags swapped
    assert ps == ps2
    np.testing.assert_allclose(dps[:2], dps2[2:], rtol=1e-15)
    assert abs(dps.sum()) <= 1e-16                                # equal and opposite
    d = t[:2].mean() - t[2:].mean()
    assert abs(ps - np.exp(-d * d / 2)) <= 1e-16
    # one group: no push; no group: nothing
    assert ref.image_loss(t, np.zeros(4, int))[1] == 0.0
    assert ref.image_loss([], [])[:2] == (0.0, 0.0)


def test_slots_outside_a_group_are_never_read():
    tags, pts, gid, H, W = _case(5)
    gid[0, 0, 0], gid[0, 1, 1] = -1, 32
    pts[1, 2, 2, 2] = 0
    base = ref.tag_loss(tags, pts, gid, H, W)
    pts2 = pts.copy()
    pts2[0, 0, 0, :2] = np.nan
    pts2[0, 1, 1, :2] = np.inf
    pts2[1, 2, 2, :2] = np.nan
    again = ref.tag_loss(tags, pts2, gid, H, W)
    assert np.array_equal(base[0], again[0]) and np.array_equal(base[1], again[1])


# ---- grouping: the hand cases (peaks on nodes of a lattice with H = 8(h-1)+1, tags multiples of 2^-4)

@pytest.mark.parametrize("name", sorted(ref.hand_cases()))
def test_grouping_restatement_on_hand_cases(name):
    tags, peaks, counts, H, W, order, md, want, ng = ref.hand_cases()[name]
    group, tag, ngroups = ref.peaks_group(peaks, counts, tags, H, W, order, md)
    assert group.tolist() == want, (name, group.tolist())
    assert ngroups.tolist() == ng
    K, P = counts.shape[1], peaks.shape[2]
    for c in range(K):
        for j in range(P):
            if j < min(max(counts[0, c], 0), P):
                i, jj = int(peaks[0, c, j, 1]) // 8, int(peaks[0, c, j, 0]) // 8
                assert tag[0, c, j] == tags[0, c, i, jj] or (np.isnan(tag[0, c, j]) and np.isnan(tags[0, c, i, jj]))
            else:
                assert tag[0, c, j] == 0


# ---- hkp.grouping

def test_slot_groups_written_out():
    from hkp.grouping import slot_groups
    g = slot_groups(2, 3, 4, (2, 0), "cpu")
    assert g.dtype == torch.int32 and g.tolist() == [[[0, 1, 2, 3], [-1] * 4, [0, 1, 2, 3]]] * 2
    assert slot_groups(2, 3, 4, (2, 0), "cpu") is g                    # built once
    assert slot_groups(2, 3, 4, (0, 2), "cpu") is not g
    for bad in ((), (3,), (0, 0), (-1,), (True,), (1.0,)):
        with pytest.raises(ValueError):
            slot_groups(2, 3, 4, bad, "cpu")
    with pytest.raises(ValueError):
        slot_groups(2, 3, 17, (0,), "cpu")


def test_pair_scores_written_out():
    from hkp.grouping import pair_scores
    # one image, K = 2 (cap, tail), M = 2 cables, P = 2 peaks
    gid = np.array([[[0, 1], [0, 1]]])
    # every label matched: cap slot 0 -> peak 0, cap slot 1 -> peak 1; tail slot 0 -> peak 1, tail slot 1 -> peak 0
    gt_match = np.array([[[0, 1], [1, 0]]])
    right = np.array([[[0, 1], [1, 0]]])           # tail peak 1 is with cap peak 0: the cables are whole
    assert pair_scores(right, gt_match, gid) == dict(label_groups=2, paired=1.0, pred_groups=2, mixed=0.0)
    wrong = np.array([[[0, 1], [0, 1]]])           # tail peak 0 (cable 1) grouped with cap peak 0 (cable 0)
    assert pair_scores(wrong, gt_match, gid) == dict(label_groups=2, paired=0.0, pred_groups=2, mixed=1.0)
    # a missed tail: that cable has one matched member and does not count; an ungrouped peak pairs nothing
    miss = np.array([[[0, 1], [1, -1]]])
    assert pair_scores(right, miss, gid) == dict(label_groups=1, paired=1.0, pred_groups=2, mixed=0.0)
    none = np.array([[[0, 1], [-1, -1]]])
    assert pair_scores(none, gt_match, gid) == dict(label_groups=2, paired=0.0, pred_groups=2, mixed=0.0)
    # labels outside a group, empty slots (-2) and tensors
    gid2 = np.array([[[0, -1], [0, 32]]])
    got = pair_scores(torch.tensor(right), torch.tensor([[[0, -2], [1, -2]]]), torch.tensor(gid2))
    assert got == dict(label_groups=1, paired=1.0, pred_groups=1, mixed=0.0)
    assert pair_scores(right, np.full((1, 2, 2), -1), gid) == dict(label_groups=0, paired=0.0, pred_groups=0, mixed=0.0)
    with pytest.raises(ValueError):
        pair_scores(right, gt_match[:, :1], gid)


# ---- rejections

def _ops_args(K=2, M=3, P=4, h=3, w=4):
    low = torch.zeros(2, 2 * K, h, w)
    return dict(low=low, pts=torch.zeros(2, K, M, 3), gid=torch.zeros(2, K, M, dtype=torch.int32),
                peaks=torch.zeros(2, K, P, 3), counts=torch.zeros(2, K, dtype=torch.int32))


def test_ops_reject_before_a_tensor_is_touched():
    """Every argument error is raised on shapes and numbers alone; tensors that pass them
    (here on the CPU) are then refused for their device — nothing is launched."""
    from hkp import ops
    from hkp._lib import HkpError
    a = _ops_args()
    tl = lambda **kw: ops.tag_loss(kw.pop("low", a["low"]), kw.pop("pts", a["pts"]), kw.pop("gid", a["gid"]),  # noqa: E731
                                   kw.pop("H", 17), kw.pop("W", 25), kw.pop("scale", 1e-3), **kw)
    for kw, msg in ((dict(low=torch.zeros(2, 5, 3, 4)), "2K"), (dict(low=torch.zeros(2, 18, 3, 4)), "2K"),
                    (dict(low=torch.zeros(2, 4, 0, 4)), "non-empty"), (dict(low=None), "low_all"),
                    (dict(H=0), "picture size"), (dict(scale=-1.0), "scale"), (dict(scale=float("nan")), "scale"),
                    (dict(scale=float("inf")), "scale"), (dict(scale=1e39), "scale"), (dict(pull=-0.5), "pull"),
                    (dict(push=float("nan")), "push"), (dict(pts=torch.zeros(2, 3, 3, 3)), "pts"),
                    (dict(pts=torch.zeros(2, 2, 17, 3)), "pts"), (dict(pts=torch.zeros(2, 2, 3, 2)), "pts"),
                    (dict(gid=torch.zeros(2, 2, 4, dtype=torch.int32)), "gid"), (dict(gid=None), "gid"),
                    (dict(dtag=torch.zeros(2, 2, 3, 5)), "dtag"),
                    (dict(dtag=torch.zeros(2, 2, 3, 4), want_grad=False), "dtag"),
                    (dict(), "on the GPU"), (dict(gid=a["gid"].long()), "on the GPU")):
        with pytest.raises(HkpError, match=msg):
            tl(**kw)
    pg = lambda **kw: ops.peaks_group(kw.pop("peaks", a["peaks"]), kw.pop("counts", a["counts"]),  # noqa: E731
                                      kw.pop("low", a["low"]), kw.pop("H", 17), kw.pop("W", 25),
                                      kw.pop("order", (0, 1)), **kw)
    for kw, msg in ((dict(low=torch.zeros(2, 3, 3, 4)), "2K"), (dict(W=0), "picture size"), (dict(order=()), "order"),
                    (dict(order=(0, 1, 0)), "order"), (dict(order=(0, 0)), "twice"), (dict(order=(2,)), "no class"),
                    (dict(order=(-1,)), "no class"), (dict(order=(0.0,)), "no class"), (dict(order=3), "sequence"),
                    (dict(max_dist=0.0), "max_dist"), (dict(max_dist=float("inf")), "max_dist"),
                    (dict(max_dist=float("nan")), "max_dist"), (dict(peaks=torch.zeros(2, 2, 17, 3)), "peaks"),
                    (dict(peaks=torch.zeros(2, 3, 4, 3)), "peaks"), (dict(counts=torch.zeros(2, 3)), "counts"),
                    (dict(), "on the GPU")):
        with pytest.raises(HkpError, match=msg):
            pg(**kw)


def test_net_and_trainer_reject_tags_that_do_not_fit():
    from hkp import net, ops
    from hkp.train import Trainer
    with pytest.raises(ops.HkpError, match="2K"):
        net.keypoints_forward(None, None, 9, tags=True)                # raised before anything is read

    class _M:
        num_keypoints = 9
    for k, tags in ((9, {"classes": (0,)}), (4, {"classes": (4,)}), (4, {"classes": ()}), (4, {"classes": (1, 1)}),
                    (4, {"weight": 1.0}), (4, {"classes": (0,), "weights": 1.0}), (4, {"classes": (0,), "weight": -1}),
                    (4, ("cap",)), (4, {"classes": ("cap",)})):
        with pytest.raises(ValueError):
            Trainer._tags_choice(tags, k)
    assert Trainer._tags_choice(None, 99) is None
    got = Trainer._tags_choice({"classes": [1, 0]}, 4)
    assert got["classes"] == (1, 0) and got["pull"] == 1.0 and got["push"] == 1.0
    assert got["weight"] == ctypes.c_float(1e-3).value                # HigherHRNet's


def test_c_entries_reject_without_a_gpu_and_leave_outputs_alone():
    from hkp import _lib
    L = _lib.lib()
    n, k, m, p, h, w, H, W = 2, 2, 3, 4, 3, 4, 17, 25
    tags = np.zeros((n, 2 * k, h, w), np.float32)
    pts = np.zeros((n, k, m, 3), np.float32)
    gid = np.zeros((n, k, m), np.int32)
    out = np.full(3, 7.0)
    dtag = np.full((n, k, h, w), 7.0, np.float32)
    ws = np.full(2 * n, 7.0)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    good = dict(n=n, k=k, m=m, h=h, w=w, H=H, W=W, tags=P(tags), stride=2 * k * h * w, pts=P(pts), gid=P(gid), scale=1e-3,
                pull=1.0, push=1.0, out=P(out), dtag=P(dtag), ws=P(ws))
    assert L.hkp_tag_loss_workspace(n) == 16 * n and L.hkp_tag_loss_workspace(0) == 0
    bad = [dict(n=0), dict(k=0), dict(k=9), dict(m=0), dict(m=17), dict(h=0), dict(w=0), dict(H=0), dict(W=0),
           dict(h=32768), dict(w=32768), dict(tags=None), dict(pts=None), dict(gid=None), dict(out=None), dict(ws=None),
           dict(stride=k * h * w - 1), dict(scale=-1.0), dict(scale=float("nan")), dict(scale=float("inf")),
           dict(pull=-1.0), dict(pull=float("nan")), dict(push=float("inf")), dict(push=-0.5)]
    for b in bad:
        a = dict(good, **b)
        rc = L.hkp_tag_loss(a["n"], a["k"], a["m"], a["h"], a["w"], a["H"], a["W"], a["tags"], a["stride"], a["pts"],
                            a["gid"], a["scale"], a["pull"], a["push"], a["out"], a["dtag"], a["ws"], None)
        assert rc == -1, b
        assert L.hkp_last_error().decode().startswith("hkp_tag_loss"), b
    assert (out == 7).all() and (dtag == 7).all() and (ws == 7).all()

    peaks = np.zeros((n, k, p, 3), np.float32)
    counts = np.zeros((n, k), np.int32)
    tag = np.full((n, k, p), 7.0, np.float32)
    group = np.full((n, k, p), 7, np.int32)
    ngroups = np.full(n, 7, np.int32)
    order = (ctypes.c_int32 * 8)(0, 1)
    good = dict(n=n, k=k, p=p, h=h, w=w, H=H, W=W, q=2, order=order, md=1.0, peaks=P(peaks), counts=P(counts),
                tags=P(tags), stride=2 * k * h * w, tag=P(tag), group=P(group), ngroups=P(ngroups))
    bad = [dict(n=0), dict(k=0), dict(k=9), dict(p=0), dict(p=17), dict(h=0), dict(w=32768), dict(H=0), dict(W=0),
           dict(q=0), dict(q=3), dict(order=None), dict(order=(ctypes.c_int32 * 8)(0, 0)),
           dict(order=(ctypes.c_int32 * 8)(0, 2)), dict(order=(ctypes.c_int32 * 8)(-1, 0)), dict(md=0.0), dict(md=-1.0),
           dict(md=float("nan")), dict(md=float("inf")), dict(peaks=None), dict(counts=None), dict(tags=None),
           dict(tag=None), dict(group=None), dict(ngroups=None), dict(stride=k * h * w - 1)]
    for b in bad:
        a = dict(good, **b)
        rc = L.hkp_peaks_group(a["n"], a["k"], a["p"], a["h"], a["w"], a["H"], a["W"], a["q"], a["order"], a["md"],
                               a["peaks"], a["counts"], a["tags"], a["stride"], a["tag"], a["group"], a["ngroups"], None)
        assert rc == -1, b
        assert L.hkp_last_error().decode().startswith("hkp_peaks_group"), b
    assert (tag == 7).all() and (group == 7).all() and (ngroups == 7).all()


def test_defaults_are_off():
    import inspect
    import config
    from hkp import net
    from hkp.train import Trainer
    assert config.TAGS is None
    assert inspect.signature(net.keypoints_forward).parameters["tags"].default is False
    assert inspect.signature(net.keypoints_backward).parameters["dtag"].default is None
    assert inspect.signature(Trainer.__init__).parameters["tags"].default is None
