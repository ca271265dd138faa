"""Associative-embedding tags on the GPU: hkp_tag_loss and hkp_peaks_group against
their numpy restatement (tests/_tags_ref.py) at every size the kernels take another
path, in place and off alignment, and the layers above them — the 2K-row head, the
Trainer, predict_groups, train.py's fit() and analysis.py — on R18-8s at 96x128 with
synthetic scenes of two cables."""
import numpy as np
import pytest
import torch

import _tags_ref as ref
from oracle import recipe

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


# ------------------------------------------------------------------ the loss ----
LOSS_SHAPES = [(1, 1, 1, 1, 1, 1, 1), (1, 2, 2, 2, 2, 9, 9), (2, 4, 3, 5, 7, 33, 49), (2, 8, 16, 12, 16, 96, 128),
               (3, 4, 4, 60, 80, 480, 640)]


def _loss_case(shape, seed):
    """low_all [B,2K,h,w] (heat channels filled too: they must not be read) and seeded labels
    with the edge cases the shape has room for."""
    B, K, M, h, w, H, W = shape
    rng = np.random.default_rng(seed)
    low = rng.normal(0, 1.5, (B, 2 * K, h, w)).astype(np.float32)
    pts = np.zeros((B, K, M, 3), np.float32)
    pts[..., 0] = rng.uniform(-2, W + 1, (B, K, M))            # some outside the picture: clamped
    pts[..., 1] = rng.uniform(-2, H + 1, (B, K, M))
    pts[..., 2] = rng.random((B, K, M)) < 0.85
    gid = rng.integers(0, max(2, min(6, M + 1)), (B, K, M)).astype(np.int32)
    pts[0, 0, 0] = (0, 0, 1)                                    # the first node
    if M >= 2:
        pts[0, 0, 1] = (W - 1, H - 1, 1)                        # exactly on the last row and column
        pts[0, K - 1, 0] = (0.4 * W, 0.4 * H, 1)                # two points of one class in one cell ...
        pts[0, K - 1, 1] = (0.4 * W + 0.5, 0.4 * H + 0.25, 1)
        gid[0, K - 1, :2] = (0, 1)
    if K >= 2 and M >= 2:
        pts[0, 1, 0] = pts[0, 0, 1]                             # ... and two groups at the same position
        gid[0, 0, 1], gid[0, 1, 0] = 2, 3
    if M >= 3:
        gid[0, 0, 2], pts[0, 0, 2, 2] = 7, 1                    # a group of one
    if K * M >= 32:
        gid[0] = (np.arange(K * M) % 32).reshape(K, M)          # all 32 ids in use (each four times)
        pts[0, :, :, 2] = 1
    if B >= 2:
        pts[B - 1, :, :, 2] = 0                                 # an image without a group
    if B >= 3:
        gid[1] = 5                                              # an image with one group: push exactly 0
    if M >= 3:
        # last of all, so that nothing above overwrites them: live slots (flag 1) outside a group, gid -1 and
        # 32, holding NaN; they are not read.  Image 0 keeps its labels in every shape; image 1 of B >= 3 too
        pts[0, K - 1, 2], gid[0, K - 1, 2] = (np.nan, np.nan, 1), -1
        pts[0, K - 2, 2], gid[0, K - 2, 2] = (np.nan, np.nan, 1), 32
        if B >= 3:
            pts[1, K - 1, 2], gid[1, K - 1, 2] = (np.nan, np.nan, 1), 32
            pts[1, K - 2, 2], gid[1, K - 2, 2] = (np.nan, np.nan, 1), -1
    empty = pts[..., 2] <= 0
    pts[empty, 0], pts[empty, 1] = np.nan, np.nan               # empty slots hold NaN
    return low, pts, gid


def test_loss_cases_hold_what_they_claim():
    """On the host: the seeded labels reach the kernel with the cases their comments name."""
    for shape in LOSS_SHAPES:
        B, K, M, h, w, H, W = shape
        _, pts, gid = _loss_case(shape, 100 + B * K * M)
        live = pts[..., 2] > 0
        part = live & (gid >= 0) & (gid < 32)
        assert not np.isnan(pts[part][:, :2]).any(), shape         # every participating slot has coordinates
        assert np.isnan(pts[~live][:, :2]).all(), shape
        if M >= 3:                                                  # live slots with gid -1 and 32, holding NaN
            for bad in (-1, 32):
                sel = live & (gid == bad)
                assert sel.any() and np.isnan(pts[sel][:, :2]).all(), (shape, bad)
            assert (part[0] & (gid[0] == 7)).sum() == 1 or K * M >= 32
        if K * M >= 32:
            assert set(gid[0][part[0]].tolist()) == set(range(32)), shape
        if B >= 2:
            assert not part[B - 1].any()
        if B >= 3:
            assert set(gid[1][part[1]].tolist()) == {5}


def _ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def _check_loss(out, dtag, r_out, r_dtag):
    out, dtag = out.cpu().numpy(), dtag.cpu().numpy().astype(np.float64)
    for i in range(3):
        print("out[%d] gpu %.17g ref %.17g" % (i, out[i], r_out[i]))
        if r_out[i] == 0:
            assert out[i] == 0
        else:
            assert abs(out[i] - r_out[i]) <= 2.0 ** -40 * abs(r_out[i])
    for b in range(dtag.shape[0]):
        bound = _ulp32(r_dtag[b]) + 2.0 ** -40 * np.abs(r_dtag[b]).max()
        err = np.abs(dtag[b] - r_dtag[b])
        print("image %d: max |dtag - ref| %.3g, max |ref| %.3g, worst err / bound %.3g"
              % (b, err.max(), np.abs(r_dtag[b]).max(), (err / bound).max()))
        assert (err <= bound).all()


@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tag_loss_matches_the_restatement(cuda_device, shape):
    from hkp import ops
    B, K, M, h, w, H, W = shape
    low, pts, gid = _loss_case(shape, 100 + B * K * M)
    scale, pull, push = 0.75, 1.0, 0.5
    r_out, r_dtag = ref.tag_loss(low[:, K:], pts, gid, H, W, scale, pull, push)
    if B >= 3:
        assert ref.tag_loss(low[1:2, K:], pts[1:2], gid[1:2], H, W)[0][2] == 0.0      # one group: push exactly 0
    with torch.cuda.device(cuda_device):
        d_low, d_pts, d_gid = (torch.from_numpy(a).to(cuda_device) for a in (low, pts, gid))
        out, dtag = ops.tag_loss(d_low, d_pts, d_gid, H, W, scale, pull, push)         # the tag planes in place
        _check_loss(out, dtag, r_out, r_dtag)
        if B >= 2:
            assert not dtag[B - 1].any() and not torch.signbit(dtag[B - 1]).any()      # no group: +0 everywhere
        # a second run, a run without dtag, and a run into a dtag that held NaN: the same bits
        out2, dtag2 = ops.tag_loss(d_low, d_pts, d_gid, H, W, scale, pull, push)
        out3, none = ops.tag_loss(d_low, d_pts, d_gid, H, W, scale, pull, push, want_grad=False)
        pre = torch.full_like(dtag, float("nan"))
        out4, dtag4 = ops.tag_loss(d_low, d_pts, d_gid, H, W, scale, pull, push, dtag=pre)
        assert none is None and dtag4 is pre
        for o in (out2, out3, out4):
            assert torch.equal(_bits(o), _bits(out))
        assert torch.equal(_bits(dtag2), _bits(dtag)) and torch.equal(_bits(dtag4), _bits(dtag))
        # scale 0: an all-zero dtag, the same three values
        out0, dtag0 = ops.tag_loss(d_low, d_pts, d_gid, H, W, 0.0, pull, push)
        assert torch.equal(_bits(out0), _bits(out)) and not dtag0.any()
        # once more from a base 4 bytes off a 16-byte boundary, dtag 12 bytes off one, guards around it
        n_low, n_dt = d_low.numel(), dtag.numel()
        buf = torch.zeros(n_low + 8, device=cuda_device)
        off_low = buf[1:1 + n_low].view_as(d_low)
        off_low.copy_(d_low)
        guard = torch.full((n_dt + 16,), 123.0, device=cuda_device)
        off_dtag = guard[7:7 + n_dt].view_as(dtag)
        assert off_low.data_ptr() % 16 == 4 and off_dtag.data_ptr() % 16 == 12
        out5, _ = ops.tag_loss(off_low, d_pts, d_gid, H, W, scale, pull, push, dtag=off_dtag)
        assert torch.equal(_bits(out5), _bits(out)) and torch.equal(_bits(off_dtag), _bits(dtag))
        assert (guard[:7] == 123).all() and (guard[7 + n_dt:] == 123).all()


# ------------------------------------------------------------------ the grouping ----
def _call_group(dev, tags, peaks, counts, H, W, order, md):
    """ops.peaks_group on low_all = [NaN heat channels | tags]."""
    from hkp import ops
    low = np.concatenate([np.full_like(tags, np.nan), tags], 1)
    with torch.cuda.device(dev):
        g, t, n = ops.peaks_group(torch.from_numpy(peaks).to(dev), torch.from_numpy(counts).to(dev),
                                  torch.from_numpy(low).to(dev), H, W, order, max_dist=md)
    return g.cpu(), t.cpu(), n.cpu()


def _same_tags(a, b):
    return torch.equal(_bits(a), _bits(b)) or (torch.equal(torch.isnan(a), torch.isnan(b))
                                               and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)))


@pytest.mark.parametrize("name", sorted(ref.hand_cases()))
def test_peaks_group_hand_cases(cuda_device, name):
    tags, peaks, counts, H, W, order, md, want, ng = ref.hand_cases()[name]
    g, t, n = _call_group(cuda_device, tags, peaks, counts, H, W, order, md)
    assert g.tolist() == want and n.tolist() == ng, (name, g.tolist(), n.tolist())
    rg, rt, rn = ref.peaks_group(peaks, counts, tags, H, W, order, md)
    assert torch.equal(g, torch.from_numpy(rg)) and torch.equal(n, torch.from_numpy(rn))
    assert _same_tags(t, torch.from_numpy(rt))


def _node_peaks(B, K, P, h, w, seed, levels=32, full=False):
    """Tag maps of multiples of 2^-4 in [-levels/16, levels/16] and P peaks per plane on distinct nodes; counts
    between 0 and P, some -1 and P + 3; slots at and above the count hold NaN."""
    rng = np.random.default_rng(seed)
    H, W = 8 * (h - 1) + 1, 8 * (w - 1) + 1
    tags = (rng.integers(-levels, levels + 1, (B, K, h, w)) / 16.0).astype(np.float32)
    peaks = np.zeros((B, K, P, 3), np.float32)
    counts = rng.integers(0, P + 1, (B, K)).astype(np.int32)
    counts[rng.random((B, K)) < 0.15] = -1
    counts[rng.random((B, K)) < 0.3] = P + 3
    if full:
        counts[:] = P
    for b in range(B):
        for c in range(K):
            nodes = rng.permutation(h * w)[:P]
            peaks[b, c, :, 0], peaks[b, c, :, 1] = 8 * (nodes % w), 8 * (nodes // w)
            peaks[b, c, :, 2] = np.sort(rng.random(P))[::-1]
            peaks[b, c, min(max(counts[b, c], 0), P):] = np.nan
    return tags, peaks, counts, H, W


@pytest.mark.parametrize("B,K,P,h,w", [(2, 4, 4, 5, 7), (3, 8, 16, 9, 11)])
def test_peaks_group_is_exact_on_nodes(cuda_device, B, K, P, h, w):
    tags, peaks, counts, H, W = _node_peaks(B, K, P, h, w, 7 * K + P)
    rng = np.random.default_rng(K)
    seen_join = seen_open = False
    for Q in (2, 3, K):
        order = tuple(int(v) for v in rng.permutation(K)[:Q])
        for md in (0.25, 1.0):
            g, t, n = _call_group(cuda_device, tags, peaks, counts, H, W, order, md)
            rg, rt, rn = ref.peaks_group(peaks, counts, tags, H, W, order, md)
            assert torch.equal(g, torch.from_numpy(rg)), (order, md)
            assert torch.equal(n, torch.from_numpy(rn)) and torch.equal(_bits(t), _bits(torch.from_numpy(rt)))
            used = int((rg >= 0).sum())
            seen_join |= int(rn.sum()) < used
            seen_open |= int(rn.max()) > 1
            for c in set(range(K)) - set(order):
                assert (rg[:, c] == -1).all()
    assert seen_join and seen_open
    if P == 16:
        # more than 64 groups (a lane's second group), and peaks that join one of those: tags spread
        # over +-8 and every slot used
        tags, peaks, counts, H, W = _node_peaks(1, K, P, h, w, 5, levels=128, full=True)
        for md in (0.25, 2.0 ** -6):
            g, t, n = _call_group(cuda_device, tags, peaks, counts, H, W, tuple(range(K)), md)
            rg, rt, rn = ref.peaks_group(peaks, counts, tags, H, W, tuple(range(K)), md)
            assert torch.equal(g, torch.from_numpy(rg)) and torch.equal(n, torch.from_numpy(rn))
            assert torch.equal(_bits(t), _bits(torch.from_numpy(rt)))
        assert rn.max() > 64 and np.bincount(rg[rg >= 64]).max() >= 2


def test_peaks_group_tags_off_node(cuda_device):
    B, K, P, h, w, H, W = 2, 3, 5, 7, 9, 50, 70
    rng = np.random.default_rng(3)
    tags = rng.normal(0, 2, (B, K, h, w)).astype(np.float32)
    peaks = np.zeros((B, K, P, 3), np.float32)
    peaks[..., 0], peaks[..., 1] = rng.uniform(-1, W, (B, K, P)), rng.uniform(-1, H, (B, K, P))
    peaks[0, 0, 0, :2], peaks[0, 0, 1, :2] = (0, 0), (W - 1, H - 1)
    counts = np.full((B, K), P, np.int32)
    _, t, _ = _call_group(cuda_device, tags, peaks, counts, H, W, (0, 1, 2), 1.0)
    rt = ref.peaks_group(peaks, counts, tags, H, W, (0, 1, 2), 1.0)[1]
    err = np.abs(t.numpy().astype(np.float64) - rt.astype(np.float64))
    print("off-node tags: worst error in ulp32 %.3g" % (err / _ulp32(rt)).max())
    assert (err <= _ulp32(rt)).all()


# ------------------------------------------------------------------ network and layers ----
K_, HW_ = 2, (96, 128)
SCENES = dict(classes=("cap", "tail"), cables=(2, 2), blobs=(0, 2), instances=2)


def _r18(dev, seed=23):
    from src.model import KeypointsGauss
    m = KeypointsGauss(K_, HW_[0], HW_[1], backbone="resnet18", pretrained=False)
    m.load_state_dict(recipe.seeded_state_dict("resnet18", seed))
    return m.to(dev)


def _batches(dev, seed, n, bs, fixed=False):
    from hkp.synth import CableScenes
    from src.dataset import DeviceBatches, SynthDataset
    return DeviceBatches(SynthDataset(CableScenes(seed=seed, **SCENES), n, HW_, fixed=fixed, device=dev), bs, device=dev)


@pytest.fixture(scope="module")
def scene_batch(cuda_device):
    with torch.cuda.device(cuda_device):
        img, pts = next(iter(_batches(cuda_device, 31, 4, 4, fixed=True)))
    # up to two cables a picture (the sampler may place one only): some picture has both slots of both classes
    assert pts.shape == (4, K_, 2, 3) and (pts[..., 2] > 0).all(-1).all(-1).any()
    return img, pts


def test_heat_channels_do_not_depend_on_the_tag_rows(cuda_device, scene_batch):
    from hkp import net
    img, _ = scene_batch
    m = _r18(cuda_device)
    with torch.cuda.device(cuda_device), torch.no_grad():
        for traced in (True, False):
            mk = (lambda: net.Trace(m.policy)) if traced else (lambda: None)
            tr_plain, tr_tags = mk(), mk()
            hm, _, low = net.keypoints_forward(m.resnet.net, img, K_, trace=tr_plain, pol=m.policy)
            hm2, _, low_all = net.keypoints_forward(m.resnet.net, img, K_, trace=tr_tags, pol=m.policy, tags=True)
            assert low_all.shape == (4, 2 * K_, 12, 16) and low.shape == (4, K_, 12, 16)
            assert torch.equal(_bits(low_all[:, :K_]), _bits(low)), traced
            assert torch.equal(_bits(hm2), _bits(hm))
            assert low_all[:, K_:].abs().max() > 0
            if traced:
                assert tr_tags.head["low"] is low_all and tr_tags.head["tags"] and not tr_plain.head["tags"]
        none, _, low_only = net.keypoints_forward(m.resnet.net, img, K_, pol=m.policy, upsample=False, tags=True)
        assert none is None and torch.equal(_bits(low_only), _bits(low_all))


def _grads(m):
    return [p.grad.clone() for p in m.parameters()]


def test_trainer_with_tags(cuda_device, scene_batch, monkeypatch):
    from hkp import net, ops
    from hkp.grouping import slot_groups
    from hkp.train import Trainer
    img, pts = scene_batch
    m = _r18(cuda_device)
    fcw = m.resnet.net.fc.weight
    calls = []
    real = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (calls.append((name, a)), real(name, *a))[1])
    with torch.cuda.device(cuda_device):
        Trainer(m).forward_backward(img, pts=pts)              # the first step also packs the weights: not compared
        del calls[:]
        # the library calls of a step without tags: the default, and tags=None spelled out
        loss_plain = Trainer(m).forward_backward(img, pts=pts)
        plain, names_plain = _grads(m), [c[0] for c in calls]
        del calls[:]
        tr_none = Trainer(m, tags=None)
        tr_none.forward_backward(img, pts=pts)
        assert [c[0] for c in calls] == names_plain and tr_none.tag_loss is None
        assert not any("tag" in n or "group" in n for n in names_plain)
        assert [c[1][3] for c in calls if c[0] in ("hkp_head_fc", "hkp_head_fc_bwd")] == [K_, K_]
        # weight 0: every parameter gradient is the plain step's, the tag rows' exactly zero
        del calls[:]
        tr0 = Trainer(m, tags={"classes": (0, 1), "weight": 0.0})
        loss0 = tr0.forward_backward(img, pts=pts)
        names0 = [c[0] for c in calls]
        assert names0.count("hkp_tag_loss") == 1 and sorted(names0) == sorted(names_plain + ["hkp_tag_loss"])
        assert [c[1][3] for c in calls if c[0] in ("hkp_head_fc", "hkp_head_fc_bwd")] == [2 * K_, 2 * K_]
        assert torch.equal(_bits(loss0), _bits(loss_plain))
        for p, g0, g in zip(m.parameters(), _grads(m), plain):
            assert torch.equal(g0, g), tuple(p.shape)
        assert not fcw.grad[K_:].any()
        out0 = tr0.tag_loss.cpu()
        assert out0.shape == (3,) and out0.dtype == torch.float64 and out0[0] > 0
        # weight 1e-3: the step is the manual chain
        tr = Trainer(m, tags={"classes": (0, 1)})
        loss = tr.forward_backward(img, pts=pts)
        got, got_out = _grads(m), tr.tag_loss.clone()
        assert torch.equal(_bits(loss), _bits(loss_plain)) and torch.equal(_bits(got_out), _bits(tr0.tag_loss))
        trace = net.Trace(m.policy)
        hm, _, low_all = net.keypoints_forward(m.resnet.net, img, K_, heat=True, trace=trace, tags=True)
        _, dheat = ops.heat_loss_multi(hm, pts, 8.0, "bce", "zero")
        gid = slot_groups(4, K_, 2, (0, 1), cuda_device)
        out3, dtag = ops.tag_loss(low_all, pts, gid, HW_[0], HW_[1], 1e-3, 1.0, 1.0)
        grads = net.keypoints_backward(m.resnet.net, trace, dheat, net.Grads(), dtag=dtag)
        assert torch.equal(_bits(out3), _bits(got_out))
        for p, g in zip(m.parameters(), got):
            assert torch.equal(_bits(grads[p]), _bits(g)), tuple(p.shape)
        gw = grads[fcw].reshape(fcw.shape[0], -1)
        assert gw[K_:2 * K_].abs().max() > 0 and not gw[2 * K_:].any()
        assert grads[m.resnet.net.fc.bias][K_:2 * K_].abs().max() > 0 and not grads[m.resnet.net.fc.bias][2 * K_:].any()
        assert torch.equal(_bits(gw[:K_]), _bits(plain[[id(p) for p in m.parameters()].index(id(fcw))]
                                                 .reshape(fcw.shape[0], -1)[:K_]))
        # an explicit gid is used as given; labels without groups are refused before the forward
        swapped = gid.clone()
        swapped[:, 1] = gid[:, 1].flip(-1)
        tr.forward_backward(img, pts=pts, gid=swapped)
        assert not torch.equal(tr.tag_loss, got_out)
        del calls[:]
        for kw in (dict(uv=pts[:, :, 0, :2].contiguous()), dict(pts=pts, uv=pts[:, :, 0, :2].contiguous()),
                   dict(target=torch.zeros(4, K_, *HW_, dtype=torch.float64, device=cuda_device))):
            with pytest.raises(ops.HkpError, match="tags need pts"):
                tr.forward_backward(img, **kw)
        with pytest.raises(ops.HkpError, match="gid goes with"):
            tr_none.forward_backward(img, pts=pts, gid=gid)
        with pytest.raises(ops.HkpError, match="dtag goes with"):
            net.keypoints_backward(m.resnet.net, trace, dheat, net.Grads())
        with pytest.raises(ops.HkpError, match="does not go with dlow"):
            net.keypoints_backward(m.resnet.net, trace, dheat, net.Grads(), dtag=dtag[:, :1].contiguous())
        assert not calls                                       # each raised before anything was launched


def test_predict_groups(cuda_device, scene_batch):
    from hkp import net, ops
    from src.prediction import Prediction
    img, _ = scene_batch
    m = _r18(cuda_device)
    kw = dict(max_peaks=3, radius=1, threshold=0.0)
    with torch.cuda.device(cuda_device):
        peaks, counts, group, tag = m.predict_groups(img, (1, 0), max_dist=0.05, **kw)
        pk, ct = m.predict_peaks(img, **kw)
        assert torch.equal(_bits(peaks), _bits(pk)) and torch.equal(counts, ct) and int(ct.sum()) > 0
        with torch.no_grad():
            low_all = net.keypoints_forward(m.resnet.net, img, K_, pol=m.policy, upsample=False, tags=True)[2]
        pk2, ct2 = ops.heat_peaks(low_all[:, :K_].contiguous(), *HW_, **kw)
        g2, t2, _ = ops.peaks_group(pk2, ct2, low_all, *HW_, (1, 0), max_dist=0.05)
        assert torch.equal(_bits(pk2), _bits(pk)) and torch.equal(group, g2) and torch.equal(_bits(tag), _bits(t2))
        assert ((group >= 0) == (torch.arange(3, device=cuda_device)[None, None] < ct[..., None])).all()
        via = Prediction(m, K_, *HW_, True).groups(img, (1, 0), max_dist=0.05, **kw)
        assert torch.equal(via[2], group) and torch.equal(_bits(via[3]), _bits(tag))
        with pytest.raises(TypeError):
            m.predict_groups(img, (0, 1), tta=None)


def _run_main(train_mod, tmp_path, monkeypatch, capsys, tags):
    monkeypatch.chdir(tmp_path)
    for name, v in (("IMG_HEIGHT", HW_[0]), ("IMG_WIDTH", HW_[1]), ("NUM_KEYPOINTS", K_), ("batch_size", 4),
                    ("epochs", 1), ("BACKBONE", "resnet18"), ("TAGS", tags), ("_trainer", None),
                    ("SYNTH", {"train": 8, "test": 4, "seed": 5, "classes": ("cap", "tail"), "instances": 2,
                               "cables": (2, 2)})):
        monkeypatch.setattr(train_mod, name, v)
    torch.manual_seed(5)
    with pytest.warns(UserWarning, match="pretrained"):
        train_mod.main("scenes")
    # (the per-step progress `[epoch, batch] loss:` ends in "\r", which splitlines() splits at)
    return [ln for ln in capsys.readouterr().out.splitlines() if ln.strip() and not ln.startswith("[")]


def test_fit_prints_the_tag_loss_line_only_with_config_tags(cuda_device, tmp_path, monkeypatch, capsys):
    import train as train_mod
    assert train_mod.TAGS is None
    lines = _run_main(train_mod, tmp_path, monkeypatch, capsys, None)
    assert [ln.split(":")[0] for ln in lines] == ["train loss", "test loss"], lines
    lines = _run_main(train_mod, tmp_path, monkeypatch, capsys, {"classes": ("tail", "cap"), "weight": 1e-3})
    assert [ln.split(":")[0] for ln in lines] == ["train loss", "train tag loss", "test loss"], lines
    total, pull, push = (float(v) for v in lines[1].split(":")[1].split())
    print(lines[1])
    assert np.isfinite([total, pull, push]).all() and pull >= 0 and 0 <= push <= 1
    assert abs(total - (pull + push)) <= 1e-12
    assert train_mod._trainer.tags["classes"] == (1, 0)
    with pytest.raises(ValueError, match="not in config.SYNTH"):
        _run_main(train_mod, tmp_path, monkeypatch, capsys, {"classes": ("plug",)})


def test_analysis_writes_peak_groups(tmp_path, monkeypatch, cuda_device):
    import analysis as analysis_mod
    from PIL import Image
    from src.dataset import transform
    cfg = {"max_peaks": 3, "radius": 1, "threshold": 0.0}
    for name, v in (("IMG_HEIGHT", HW_[0]), ("IMG_WIDTH", HW_[1]), ("BACKBONE", "resnet18"), ("NUM_KEYPOINTS", K_)):
        monkeypatch.setattr(analysis_mod, name, v)
    sd = recipe.seeded_state_dict("resnet18", 91)
    (tmp_path / "ck").mkdir()
    torch.save(sd, tmp_path / "ck" / "m.pth")
    (tmp_path / "imgs").mkdir()
    srcs = [recipe.seeded_images_u8(1, *HW_, 92 + i)[0] for i in range(2)]
    for i, bgr in enumerate(srcs):
        Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(tmp_path / "imgs" / ("f%d.png" % i))
    run = lambda out: analysis_mod.main("m.pth", str(tmp_path / "imgs"), out_dir=str(tmp_path / out),    # noqa: E731
                                        checkpoint_dir=str(tmp_path / "ck"))
    monkeypatch.setattr(analysis_mod, "PEAKS", cfg)
    kp_plain = run("plain")
    assert not (tmp_path / "plain" / "peak_groups.npy").exists()
    monkeypatch.setattr(analysis_mod, "PEAKS", dict(cfg, groups={"classes": (0, 1), "max_dist": 0.05}))
    kp = run("preds")
    assert np.array_equal(kp, kp_plain)
    for f in ("keypoints.npy", "peaks.npy", "peak_counts.npy"):
        assert np.array_equal(np.load(tmp_path / "preds" / f), np.load(tmp_path / "plain" / f)), f
    groups = np.load(tmp_path / "preds" / "peak_groups.npy")
    assert groups.shape == (2, K_, 3) and groups.dtype == np.int32
    m = _r18(cuda_device, 91)
    for i, frame in enumerate(srcs):
        g = m.predict_groups(transform(frame).to(cuda_device)[None], (0, 1), max_dist=0.05, **cfg)[2]
        assert np.array_equal(groups[i:i + 1], g.cpu().numpy()), i
    assert (groups >= 0).any()
    monkeypatch.setattr(analysis_mod, "PEAKS", dict(cfg, groups={"classes": (0, 1)}, tta={"hflip": True}))
    with pytest.raises(ValueError, match="does not go with 'tta'"):
        run("bad")


def test_training_lowers_the_held_out_tag_loss(cuda_device):
    """R18-8s, 96x128, two cables, tags on (cap, tail): STEPS Trainer steps of batch 8 on fresh
    scenes must leave the mean tag loss (pull + push, weights 1) of 16 fixed held-out scenes
    below its value at initialisation, where all tags are nearly equal and the loss is close
    to push_w = 1.  Measured on the MI355X: see the README's tags section."""
    from hkp import net, ops
    from hkp.grouping import slot_groups
    from hkp.train import Trainer
    STEPS = 48
    m = _r18(cuda_device)
    with torch.cuda.device(cuda_device):
        h_img, h_pts = next(iter(_batches(cuda_device, 11, 16, 16, fixed=True)))
        gid = slot_groups(16, K_, 2, (0, 1), cuda_device)

        def held_out():
            with torch.no_grad():
                low_all = net.keypoints_forward(m.resnet.net, h_img, K_, pol=m.policy, upsample=False, tags=True)[2]
            return ops.tag_loss(low_all, h_pts, gid, *HW_, 1.0, want_grad=False)[0].tolist()

        before = held_out()
        tr = Trainer(m, tags={"classes": (0, 1)})
        for img, pts in _batches(cuda_device, 10, 8 * STEPS, 8):
            tr.step(img, pts=pts)
        after = held_out()
    print("held-out tag loss (total, pull, push) before %r after %r; last train %r"
          % (before, after, tr.tag_loss.tolist()))
    assert np.isfinite(after[0]) and after[0] < before[0]
