"""hkp_heat_loss_planes on the GPU: plane weights, the per-plane loss values and hard
keypoint mining (top-k) against the float64 reference of tests/_planes_ref.py, against
hkp_heat_loss_multi_ex bit for bit where the two agree by definition, and through the layers
above it (ops, autograd, Trainer, train.fit).

Shapes, labels and heat are those of tests/test_gpu_instances.py (imported): the scalar and
the 16-byte path, a misaligned base, fewer elements than a block, several trips, M = 16,
absent planes, NaN in empty slots.  The top-k shapes add K = 4, 5, 6 and 64.  The dense
target comes from the existing target kernel (pinned by test_gpu_instances.py).  Each
figure is printed before it is asserted (pytest -s)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _planes_ref as pref
from oracle import recipe
from test_gpu_focal import (_differ, _labels, _loss_bound, _plus_zero, _r18, _saturated, _within_one_ulp,
                            _write_split)
from test_gpu_instances import SHAPES, _heat, _points, _same_bits

pytestmark = pytest.mark.gpu

NAN = float("nan")
ABSENT = ["zero", "ignore"]
NORMS = ["elements", "instances"]
KINDS = [("bce", 2.0), ("mse", 2.0), ("qfl", 2.0), ("qfl", 1.5)]
TOPK_SHAPES = [(2, 5, 2, 17, 23), (2, 6, 3, 12, 40), (1, 4, 1, 75, 101), (1, 64, 1, 5, 7)]


def _weights(shape):
    n, k = shape[:2]
    return torch.rand(n, k, generator=torch.Generator().manual_seed(9)) * 1.5 + 0.25


@functools.lru_cache(maxsize=None)
def _target_of(shape, absent, sigma):
    """The dense fp64 target of a shape's labels from the existing target kernel, on the
    CPU; computed once per case and left unchanged."""
    from hkp import ops
    H, W = shape[3:]
    return ops.gauss_target_multi(_labels(shape, absent).cuda(), H, W, sigma).cpu()


def _ref(shape, absent, norm, kind, beta, sigma=8.0, weights=None, topk=None, heat=None):
    return pref.planes_ref(_heat(shape) if heat is None else heat, _target_of(shape, absent, sigma),
                           _labels(shape, absent), kind, absent, norm, beta, weights, topk)


def _close(what, got, want, total):
    err, bound = abs(got - want), _loss_bound(total, want)
    print("%s: loss %.17g ref %.17g err %.3e bound %.3e" % (what, got, want, err, bound))
    assert np.isfinite(got) and err <= bound, (what, err, bound)


def _planes_close(what, got, want, hw):
    """plane_loss against the reference's: -1 in the same places, the others within the
    loss bound of a plane's hw elements."""
    got, want = got.cpu(), want.cpu()
    err = (got - want).abs().max().item()
    print("%s: plane_loss worst error %.3e" % (what, err))
    assert torch.equal(got == -1, want == -1) and ((got - want).abs() <= (hw + 16) * 2.0 ** -53 * want.abs()).all()


def _bits64(t):
    return t.detach().cpu().numpy().view(np.int64)


def _ex(pd, ptsd, kind, absent, norm, beta, sigma=8.0):
    """hkp_heat_loss_multi_ex itself (ops.heat_loss_multi sends BCE / MSE with the elements
    divisor to hkp_heat_loss_multi)."""
    from hkp import _lib, ops
    n, k, H, W = pd.shape
    P = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731
    ws = torch.empty(_lib.lib().hkp_heat_loss_multi_workspace(n, k, H, W) // 8, device=pd.device, dtype=torch.float64)
    loss = torch.full((), NAN, device=pd.device, dtype=torch.float64)
    g = torch.full_like(pd, NAN)
    _lib.call("hkp_heat_loss_multi_ex", n, k, ptsd.shape[2], H, W, {"bce": 0, "mse": 1, "qfl": 2}[kind],
              0 if absent == "zero" else 1, 0 if norm == "elements" else 1, beta, P(pd), P(ptsd), sigma, P(loss), P(g),
              P(ws), ops._stream())
    return loss, g


# ----------------------------------------------------- 1. the bits of the existing entry ----

def _check_same_as_ex(what, pd, pts, absent, norm, sigma=8.0):
    from hkp import ops
    n, k, H, W = pd.shape
    ptsd = pts.to(pd.device)
    el = pref.eligible(pts, absent)
    D = pref.divisor(pts, H, W, el, norm)
    total = int(el.sum()) * H * W
    for kind, beta in KINDS:
        tag = "%s %s %g %s %s" % (what, kind, beta, absent, norm)
        l_ex, g_ex = _ex(pd, ptsd, kind, absent, norm, beta, sigma)
        loss, dheat, plane_loss, plane_used = ops.heat_loss_planes(pd, ptsd, sigma, kind, absent, beta=beta, norm=norm)
        assert loss.dtype == torch.float64 and dheat.dtype == torch.float32 and dheat.shape == pd.shape
        assert plane_loss.dtype == torch.float64 and plane_used.dtype == torch.int32
        assert plane_loss.shape == (n, k) and plane_used.shape == (n, k)
        _same_bits(tag, dheat, g_ex)
        _close(tag, loss.item(), l_ex.item(), total)
        assert torch.equal(plane_used.cpu().bool(), el) and set(plane_used.cpu().unique().tolist()) <= {0, 1}
        pl = plane_loss.cpu()
        assert (pl[~el] == -1).all() and (pl[el] >= 0).all()
        again = (pl[el] * float(H * W)).sum().item() / D if total else 0.0
        _close(tag + " from plane_loss", again, loss.item(), total)
        if absent == "ignore":
            assert _plus_zero(dheat.cpu()[~el])
    return el


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("absent", ABSENT)
@pytest.mark.parametrize("shape", SHAPES)
def test_without_weights_and_topk_the_bits_of_multi_ex(cuda_device, shape, absent, norm):
    el = _check_same_as_ex(str(shape), _heat(shape).to(cuda_device), _labels(shape, absent), absent, norm)
    assert absent == "zero" or (~el).any() or shape[0] * shape[1] == 1


@pytest.mark.parametrize("absent", ABSENT)
def test_unaligned_base_takes_the_scalar_path(cuda_device, absent):
    """W % 4 == 0 but the heatmaps start 4 bytes off a 16-byte boundary."""
    from hkp import ops
    shape = SHAPES[4]
    p = _heat(shape).to(cuda_device)
    buf = torch.empty(p.numel() + 1, device=cuda_device)
    off = buf[1:].view(p.shape)
    off.copy_(p)
    assert off.is_contiguous() and off.data_ptr() % 16 == 4 and p.data_ptr() % 16 == 0
    pts = _labels(shape, absent)
    _check_same_as_ex("unaligned", off, pts, absent, "elements")
    w = _weights(shape).to(cuda_device)
    for topk in (None, 1):
        l1, g1, pl1, u1 = ops.heat_loss_planes(p, pts.to(cuda_device), absent=absent, weights=w, topk=topk)
        l2, g2, pl2, u2 = ops.heat_loss_planes(off, pts.to(cuda_device), absent=absent, weights=w, topk=topk)
        _same_bits("unaligned vs aligned, topk %s" % topk, g2, g1)
        _close("unaligned vs aligned, topk %s" % topk, l2.item(), l1.item(), p.numel())
        assert torch.equal(u1, u2)


# ------------------------------------------------------------------ 2. weights of one ----

@pytest.mark.parametrize("absent", ABSENT)
@pytest.mark.parametrize("shape", SHAPES)
def test_weights_of_one_give_the_bits_of_no_weights(cuda_device, shape, absent):
    from hkp import ops
    pd, ptsd = _heat(shape).to(cuda_device), _labels(shape, absent).to(cuda_device)
    ones = torch.ones(shape[:2], device=cuda_device)
    for kind, beta in KINDS:
        for norm in NORMS:
            a = ops.heat_loss_planes(pd, ptsd, 8.0, kind, absent, beta=beta, norm=norm)
            b = ops.heat_loss_planes(pd, ptsd, 8.0, kind, absent, beta=beta, norm=norm, weights=ones)
            _same_bits("weights of one %s %s %s %s" % (kind, absent, norm, shape), b[1], a[1])
            assert np.array_equal(_bits64(a[0]), _bits64(b[0])) and np.array_equal(_bits64(a[2]), _bits64(b[2]))
            assert torch.equal(a[3], b[3])


# ------------------------------------------------------------------ 3. random weights ----

@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("absent", ABSENT)
@pytest.mark.parametrize("shape", SHAPES)
def test_random_weights_against_the_reference(cuda_device, shape, absent, norm):
    from hkp import ops
    w = _weights(shape)
    pd, ptsd, wd = _heat(shape).to(cuda_device), _labels(shape, absent).to(cuda_device), w.to(cuda_device)
    for kind, beta in KINDS:
        ref = _ref(shape, absent, norm, kind, beta, weights=w)
        what = "weights %s %g %s %s %s" % (kind, beta, absent, norm, shape)
        loss, dheat, plane_loss, plane_used = ops.heat_loss_planes(pd, ptsd, 8.0, kind, absent, beta=beta, norm=norm,
                                                                   weights=wd)
        _within_one_ulp(what, dheat, ref["dheat"])
        _close(what, loss.item(), ref["loss"], ref["elements"])
        assert torch.equal(plane_used.cpu().bool(), ref["used"])
        _planes_close(what, plane_loss, ref["plane_loss"], shape[3] * shape[4])
        # the same call through heat_loss_multi
        l2, g2 = ops.heat_loss_multi(pd, ptsd, 8.0, kind, absent, beta=beta, norm=norm, weights=wd)
        assert np.array_equal(_bits64(l2), _bits64(loss))
        _same_bits(what + " via heat_loss_multi", g2, dheat)


def test_random_weights_saturated(cuda_device):
    from hkp import ops
    p, pts = _saturated()
    pd, ptsd = p.to(cuda_device), pts.to(cuda_device)
    y = ops.gauss_target_multi(ptsd, 100, 100, 0.75).cpu()
    w = _weights((1, 4))
    for kind, beta in KINDS:
        for absent in ABSENT:
            for norm in NORMS:
                ref = pref.planes_ref(p, y, pts, kind, absent, norm, beta, w)
                what = "saturated %s %g %s %s" % (kind, beta, absent, norm)
                loss, dheat, _, _ = ops.heat_loss_planes(pd, ptsd, 0.75, kind, absent, beta=beta, norm=norm,
                                                         weights=w.to(cuda_device))
                assert np.isfinite(loss.item()) and torch.isfinite(dheat).all() and torch.isfinite(ref["dheat"]).all()
                _within_one_ulp(what, dheat, ref["dheat"])
                _close(what, loss.item(), ref["loss"], ref["elements"])
                assert ref["loss"] > 0


# --------------------------------------------------------------- 4. unlabelled planes ----

@pytest.mark.parametrize("absent", ABSENT)
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[4]])
def test_unlabelled_planes(cuda_device, shape, absent):
    from hkp import ops
    n, k, m, H, W = shape
    w = _weights(shape)
    off = torch.zeros(n * k, dtype=torch.bool)
    for i, v in zip((1, k, n * k - 1), (0.0, -1.0, NAN)):
        w.view(-1)[i] = v
        off[i] = True
    off = off.view(n, k)
    p = _heat(shape)
    dirty = p.clone()
    dirty[off] = NAN                                            # never read into the result
    ptsd, wd = _labels(shape, absent).to(cuda_device), w.to(cuda_device)
    for kind, beta in KINDS:
        for norm in NORMS:
            ref = _ref(shape, absent, norm, kind, beta, weights=w)
            assert not ref["used"][off].any() and ref["used"].any()
            what = "unlabelled %s %g %s %s %s" % (kind, beta, absent, norm, shape)
            clean = ops.heat_loss_planes(p.to(cuda_device), ptsd, 8.0, kind, absent, beta=beta, norm=norm, weights=wd)
            loss, dheat, plane_loss, plane_used = ops.heat_loss_planes(dirty.to(cuda_device), ptsd, 8.0, kind, absent,
                                                                       beta=beta, norm=norm, weights=wd)
            assert np.isfinite(loss.item()) and np.array_equal(_bits64(loss), _bits64(clean[0]))
            _same_bits(what + " with NaN heat", dheat, clean[1])
            assert _plus_zero(dheat.cpu()[off]) and (plane_loss.cpu()[off] == -1).all()
            assert torch.equal(plane_used.cpu().bool(), ref["used"])
            _close(what, loss.item(), ref["loss"], ref["elements"])           # the divisor follows the reference
            _within_one_ulp(what, dheat, ref["dheat"])
    for bad in (0.0, -2.0, NAN):
        for norm in NORMS:
            none = torch.full((n, k), bad, device=cuda_device)
            loss, dheat, plane_loss, plane_used = ops.heat_loss_planes(dirty.to(cuda_device), ptsd, absent=absent,
                                                                       norm=norm, weights=none, topk=1)
            assert loss.item() == 0.0 and _plus_zero(dheat) and (plane_loss == -1).all() and not plane_used.any()
            loss, dheat, _, _ = ops.heat_loss_planes(dirty.to(cuda_device), ptsd, absent=absent, norm=norm,
                                                     weights=none)
            assert loss.item() == 0.0 and _plus_zero(dheat)


# ---------------------------------------------------------------------------- 5. top-k ----

def _topk_labels(shape, absent):
    pts = _labels(shape, absent)
    assert not (pts[:, 1, :, 2] > 0).any()                     # class 1 is absent in every image
    return pts


@pytest.mark.parametrize("sigma", [8.0, 0.75])
@pytest.mark.parametrize("kind", ["bce", "mse"])
@pytest.mark.parametrize("shape", TOPK_SHAPES[:3])
def test_topk_against_the_reference(cuda_device, shape, kind, sigma):
    from hkp import ops
    n, k, m, H, W = shape
    pd = _heat(shape, seed=4).to(cuda_device)
    for absent in ABSENT:
        pts = _topk_labels(shape, absent)
        ptsd = pts.to(cuda_device)
        for w in (None, _weights(shape)):
            wd = None if w is None else w.to(cuda_device)
            base = _ref(shape, absent, "elements", kind, 2.0, sigma, w)
            gap = pref.rank_gap(base["S"], w, base["eligible"])
            print("top-k %s %s sigma %g %s weights %s: smallest relative rank gap %.3e"
                  % (shape, kind, sigma, absent, w is not None, gap))
            assert gap > 1e-6                                   # the input's precondition, in the reference
            for norm in NORMS:
                plain = ops.heat_loss_planes(pd, ptsd, sigma, kind, absent, norm=norm, weights=wd)
                for T in (1, 2, k):
                    ref = _ref(shape, absent, norm, kind, 2.0, sigma, w, T)
                    what = "top-%d %s %s sigma %g %s %s weights %s" % (T, shape, kind, sigma, absent, norm,
                                                                       w is not None)
                    loss, dheat, plane_loss, plane_used = ops.heat_loss_planes(pd, ptsd, sigma, kind, absent, norm=norm,
                                                                               weights=wd, topk=T)
                    used = ref["used"]
                    assert torch.equal(plane_used.cpu().bool(), used), what
                    assert (used.sum(1) == torch.minimum(ref["eligible"].sum(1), torch.tensor(T))).all()
                    _close(what, loss.item(), ref["loss"], ref["elements"])
                    _within_one_ulp(what, dheat, ref["dheat"])
                    # the same gradient as the selection written into the weights
                    mask = used.float() * (1.0 if w is None else w)
                    masked = ops.heat_loss_planes(pd, ptsd, sigma, kind, absent, norm=norm,
                                                  weights=mask.to(cuda_device))
                    _same_bits(what + " vs the mask as weights", dheat, masked[1])
                    assert _plus_zero(dheat.cpu()[~used])
                    assert np.array_equal(_bits64(plane_loss), _bits64(plain[2]))        # not counted: the value stays
                    if T == k:
                        assert np.array_equal(_bits64(loss), _bits64(plain[0])) and torch.equal(plane_used, plain[3])
                        _same_bits(what + " vs topk=None", dheat, plain[1])
                    elif int(ref["eligible"].sum(1).max()) > T:
                        assert (~used & ref["eligible"]).any()


@pytest.mark.parametrize("shape", TOPK_SHAPES[:2])
def test_topk_tie_goes_to_the_lower_class(cuda_device, shape):
    from hkp import ops
    n, k, m, H, W = shape
    p, pts = _heat(shape, seed=4), _topk_labels(shape, "zero")
    p[:, k - 1], pts[:, k - 1] = p[:, 0], pts[:, 0]             # the last class is a copy of class 0
    w = torch.full((n, k), 0.01)
    w[:, 0] = w[:, k - 1] = 1.0                                 # the pair leads every image
    pd, ptsd = p.to(cuda_device), pts.to(cuda_device)
    for kind, beta in KINDS:
        for wd in (w.to(cuda_device), None):
            loss, dheat, plane_loss, plane_used = ops.heat_loss_planes(pd, ptsd, 8.0, kind, beta=beta, weights=wd,
                                                                       topk=1)
            pl = _bits64(plane_loss)
            assert np.array_equal(pl[:, 0], pl[:, k - 1])       # identical planes: identical bits
            if wd is not None:
                want = torch.zeros(n, k, dtype=torch.int32)
                want[:, 0] = 1
                assert torch.equal(plane_used.cpu(), want)
                assert _plus_zero(dheat[:, 1:]) and (dheat[:, 0] != 0).any()
                two = ops.heat_loss_planes(pd, ptsd, 8.0, kind, beta=beta, weights=wd, topk=2)
                want[:, k - 1] = 1
                assert torch.equal(two[3].cpu(), want)
                _same_bits("the tied pair's gradients", two[1][:, k - 1], two[1][:, 0])
            else:
                assert not plane_used[:, k - 1].any()           # T = 1: the copy never gets ahead of class 0


def test_topk_with_fewer_eligible_planes(cuda_device):
    from hkp import ops
    shape = TOPK_SHAPES[0]
    n, k, m, H, W = shape
    pts = _points(shape)                                        # class 1 absent, nothing else
    w = _weights(shape)
    w[0, 2:] = 0.0                                              # image 0: class 0 alone
    p = _heat(shape)
    y = ops.gauss_target_multi(pts.to(cuda_device), H, W, 8.0).cpu()
    ref = pref.planes_ref(p, y, pts, "bce", "ignore", "elements", 2.0, w, 3)
    assert ref["eligible"][0].tolist() == [True] + [False] * (k - 1) and int(ref["eligible"][1].sum()) == 4
    loss, dheat, plane_loss, plane_used = ops.heat_loss_planes(p.to(cuda_device), pts.to(cuda_device),
                                                               absent="ignore", weights=w.to(cuda_device), topk=3)
    assert torch.equal(plane_used.cpu().bool(), ref["used"]) and plane_used.sum(1).tolist() == [1, 3]
    _close("fewer eligible planes than T", loss.item(), ref["loss"], ref["elements"])
    _within_one_ulp("fewer eligible planes than T", dheat, ref["dheat"])
    _planes_close("fewer eligible planes than T", plane_loss, ref["plane_loss"], H * W)


def test_topk_with_64_classes_and_not_65(cuda_device):
    from hkp import ops
    shape = TOPK_SHAPES[3]
    n, k, m, H, W = shape
    w = _weights(shape)
    pd, ptsd = _heat(shape, seed=4).to(cuda_device), _topk_labels(shape, "zero").to(cuda_device)
    for kind in ("bce", "mse"):
        base = _ref(shape, "zero", "elements", kind, 2.0, 8.0, w)
        assert pref.rank_gap(base["S"], w, base["eligible"]) > 1e-6
        for T in (1, 2, 64):
            ref = _ref(shape, "zero", "elements", kind, 2.0, 8.0, w, T)
            loss, dheat, plane_loss, plane_used = ops.heat_loss_planes(pd, ptsd, 8.0, kind, weights=w.to(cuda_device),
                                                                       topk=T)
            assert torch.equal(plane_used.cpu().bool(), ref["used"]) and int(plane_used.sum()) == T
            _close("K = 64, top-%d %s" % (T, kind), loss.item(), ref["loss"], ref["elements"])
            _within_one_ulp("K = 64, top-%d %s" % (T, kind), dheat, ref["dheat"])
    wide, wide_pts = torch.rand(1, 65, H, W).to(cuda_device), torch.zeros(1, 65, 1, 3).to(cuda_device)
    with pytest.raises(ops.HkpError, match="at most 64"):
        ops.heat_loss_planes(wide, wide_pts, topk=2)
    loss, _, _, used = ops.heat_loss_planes(wide, wide_pts)     # without top-k any K goes
    assert np.isfinite(loss.item()) and int(used.sum()) == 65


# -------------------------------------------------------------------- 6. repeatability ----

@pytest.mark.parametrize("topk", [None, 2])
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3], SHAPES[5], TOPK_SHAPES[1]])
def test_second_run_and_missing_outputs_give_the_same_bits(cuda_device, shape, topk):
    from hkp import _lib, ops
    n, k, m, H, W = shape
    if topk is not None and k < 2:
        topk = 1
    pd, ptsd = _heat(shape).to(cuda_device), _labels(shape, "ignore").to(cuda_device)
    wd = _weights(shape).to(cuda_device)
    P = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731
    for kind, beta in KINDS:
        a = ops.heat_loss_planes(pd, ptsd, 8.0, kind, "ignore", beta=beta, weights=wd, topk=topk)
        b = ops.heat_loss_planes(pd, ptsd, 8.0, kind, "ignore", beta=beta, weights=wd, topk=topk)
        _same_bits("second run", b[1], a[1])
        assert np.array_equal(_bits64(a[0]), _bits64(b[0])) and np.array_equal(_bits64(a[2]), _bits64(b[2]))
        assert torch.equal(a[3], b[3])
        c = ops.heat_loss_planes(pd, ptsd, 8.0, kind, "ignore", want_grad=False, beta=beta, weights=wd, topk=topk)
        assert c[1] is None and np.array_equal(_bits64(a[0]), _bits64(c[0])) and torch.equal(a[3], c[3])
        # neither dheat nor the two plane outputs
        ws = torch.empty(_lib.lib().hkp_heat_loss_planes_workspace(n, k, H, W) // 8, device=cuda_device,
                         dtype=torch.float64)
        loss = torch.full((), NAN, device=cuda_device, dtype=torch.float64)
        _lib.call("hkp_heat_loss_planes", n, k, m, H, W, {"bce": 0, "mse": 1, "qfl": 2}[kind], 1, 0, beta, topk or 0,
                  P(pd), P(ptsd), P(wd), 8.0, P(loss), None, None, None, P(ws), ops._stream())
        assert np.array_equal(_bits64(a[0]), _bits64(loss))


def test_c_abi_rejects_without_writing(cuda_device):
    from hkp import _lib, ops
    shape = SHAPES[2]
    n, k, m, H, W = shape
    pd, ptsd = _heat(shape).to(cuda_device), _points(shape).to(cuda_device)
    P = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731
    ws = torch.full((_lib.lib().hkp_heat_loss_planes_workspace(n, k, H, W) // 8,), 7.0, device=cuda_device,
                    dtype=torch.float64)
    loss = torch.full((), 7.0, device=cuda_device, dtype=torch.float64)
    g = torch.full_like(pd, 7.0)
    pl = torch.full((n, k), 7.0, device=cuda_device, dtype=torch.float64)
    pu = torch.full((n, k), 7, device=cuda_device, dtype=torch.int32)
    for kind, norm, beta, topk in ((2, 0, 0.5, 0), (3, 0, 2.0, 0), (0, 2, 2.0, 0), (0, 0, 2.0, -1), (0, 0, 2.0, 2)):
        with pytest.raises(_lib.HkpError):
            _lib.call("hkp_heat_loss_planes", n, k, m, H, W, kind, 0, norm, beta, topk, P(pd), P(ptsd), None, 8.0,
                      P(loss), P(g), P(pl), P(pu), P(ws), ops._stream())
    torch.cuda.synchronize()
    assert loss.item() == 7.0 and (g == 7.0).all() and (ws == 7.0).all() and (pl == 7.0).all() and (pu == 7).all()


# ---------------------------------------------------------------- 7. defaults untouched ----

def test_calls_without_the_new_arguments_reach_what_they_reached(cuda_device, monkeypatch):
    from hkp import _lib, ops, train
    from hkp import autograd as hkp_autograd
    shape = SHAPES[4]
    n, k, m, H, W = shape
    pd, ptsd = _heat(shape).to(cuda_device), _points(shape).to(cuda_device)
    uv = ptsd[:, :, 0, :2].contiguous()
    dense = ops.gauss_target_multi(ptsd, H, W, 8.0)
    names = []
    real = ops.call
    assert real is _lib.call
    spy = lambda name, *a: (names.append(name), real(name, *a))[1]      # noqa: E731
    monkeypatch.setattr(ops, "call", spy)
    monkeypatch.setattr(_lib, "call", spy)

    def launched(fn):
        del names[:]
        fn()
        return [x for x in names if x.startswith("hkp_heat_loss") and not x.endswith("_workspace")]

    ONE, MULTI, EX, PLANES = "hkp_heat_loss", "hkp_heat_loss_multi", "hkp_heat_loss_multi_ex", "hkp_heat_loss_planes"
    assert launched(lambda: ops.heat_loss(pd, target=dense)) == [ONE]
    assert launched(lambda: ops.heat_loss(pd, uv=uv, kind="mse")) == [ONE]
    assert launched(lambda: ops.heat_loss(pd, uv=uv, kind="qfl")) == [EX]
    assert launched(lambda: ops.heat_loss_multi(pd, ptsd)) == [MULTI]
    assert launched(lambda: ops.heat_loss_multi(pd, ptsd, 8.0, "mse", "ignore", True, beta=2.0,
                                                norm="elements")) == [MULTI]
    assert launched(lambda: ops.heat_loss_multi(pd, ptsd, kind="qfl", beta=1.5)) == [EX]
    assert launched(lambda: ops.heat_loss_multi(pd, ptsd, norm="instances", weights=None, topk=None)) == [EX]
    assert launched(lambda: hkp_autograd.heatmap_loss(pd, target=dense)) == [ONE]
    assert launched(lambda: hkp_autograd.heatmap_loss(pd, uv=uv)) == [ONE]
    assert launched(lambda: hkp_autograd.heatmap_loss(pd, pts=ptsd, absent="ignore")) == [MULTI]
    assert launched(lambda: hkp_autograd.heatmap_loss(pd, pts=ptsd, kind="qfl", norm="instances")) == [EX]
    # ... and with them, the new entry alone
    w = torch.ones(n, k, device=cuda_device)
    assert launched(lambda: ops.heat_loss(pd, uv=uv, weights=w)) == [PLANES]
    assert launched(lambda: ops.heat_loss_multi(pd, ptsd, topk=1)) == [PLANES]
    assert launched(lambda: hkp_autograd.heatmap_loss(pd, pts=ptsd, return_planes=True)) == [PLANES]
    # the Trainer
    B, K, Hh, Ww = 2, 3, 64, 96
    x = recipe.to_tensor_nchw(recipe.seeded_images_u8(B, Hh, Ww, 21)).to(cuda_device)
    uv3 = torch.from_numpy(recipe.seeded_keypoints(B, K, Hh, Ww, 22)).to(cuda_device)
    pts3 = torch.cat([uv3, torch.ones(B, K, 1, device=cuda_device)], -1).reshape(B, K, 1, 3).contiguous()
    model = _r18(cuda_device, K)
    tr = train.Trainer(model)
    assert launched(lambda: tr.forward_backward(x, uv=uv3)) == [ONE] and tr.plane_loss is None
    assert launched(lambda: tr.forward_backward(x, pts=pts3)) == [MULTI] and tr.plane_used is None
    tr = train.Trainer(model, loss="qfl", loss_params={"beta": 2.0})
    assert launched(lambda: tr.forward_backward(x, pts=pts3)) == [EX]
    assert launched(lambda: tr.forward_backward(x, pts=pts3, weights=torch.ones(B, K, device=cuda_device))) == [PLANES]
    assert tr.plane_loss.shape == (B, K) and tr.plane_used.dtype == torch.int32


# --------------------------------------------------------------------------- 8. layers ----

def _step_inputs(cuda_device, B, K, H, W):
    x = recipe.to_tensor_nchw(recipe.seeded_images_u8(B, H, W, 21)).to(cuda_device)
    uv = torch.from_numpy(recipe.seeded_keypoints(B, K, H, W, 22)).to(cuda_device)
    pts = torch.cat([uv, torch.ones(B, K, 1, device=cuda_device)], -1).reshape(B, K, 1, 3).contiguous()
    pts = torch.cat([pts, torch.full_like(pts, NAN)], 2).contiguous()            # M = 2, the second slot empty
    pts[:, :, 1, 2] = 0.0
    pts[0, 1, 1] = torch.tensor([20.5, 30.25, 1.0])                               # but for one second instance
    return x, uv, pts


def test_training_step(cuda_device):
    from hkp import autograd as hkp_autograd
    from hkp import net, ops, train
    B, K, H, W = 2, 3, 64, 96
    x, uv, pts = _step_inputs(cuda_device, B, K, H, W)
    cw = (1.5, 0.5, 2.0)
    wimg = torch.tensor([[1.0, 2.0, 0.75], [0.5, 1.0, 1.25]], device=cuda_device)
    full = torch.tensor(cw, device=cuda_device)[None, :] * wimg
    m_tr, m_man, m_auto, m_zero = (_r18(cuda_device, K) for _ in range(4))
    # the manual chain
    trace = net.Trace(m_man.policy)
    hm, _, _ = net.keypoints_forward(m_man.resnet.net, x, K, heat=True, trace=trace)
    l_man, dheat, pl_man, pu_man = ops.heat_loss_planes(hm, pts, 8.0, "bce", "zero", True, weights=full, topk=2)
    grads = net.Grads()
    net.keypoints_backward(m_man.resnet.net, trace, dheat, grads)
    for p in m_man.parameters():
        p.grad = grads[p]
    assert pu_man.sum(1).tolist() == [2, 2]
    tr = train.Trainer(m_tr, loss_params={"class_weights": cw, "topk": 2})
    l_tr = tr.step(x, pts=pts, weights=wimg)
    print("Trainer planes loss %.17g, manual %.17g" % (l_tr.item(), l_man.item()))
    assert l_tr.item() == l_man.item() and np.isfinite(l_tr.item()) and l_tr.item() > 0
    differ = _differ(m_tr, m_man)
    print("parameter gradients that differ between Trainer.step and the manual chain:", differ)
    assert not differ
    assert all(torch.isfinite(q.grad).all() for q in m_tr.parameters())
    assert torch.equal(tr.plane_loss, pl_man) and torch.equal(tr.plane_used, pu_man)
    assert tr.plane_loss.is_cuda and not tr.plane_loss.requires_grad
    assert torch.equal(tr.class_weights, torch.tensor(cw, device=cuda_device))
    # the autograd path
    l_auto, pl_auto, pu_auto = hkp_autograd.heatmap_loss(m_auto(x), pts=pts, weights=full, topk=2, return_planes=True)
    assert not pl_auto.requires_grad and not pu_auto.requires_grad and l_auto.requires_grad
    l_auto.backward()
    assert l_auto.item() == l_man.item() and torch.equal(pl_auto, pl_man) and torch.equal(pu_auto, pu_man)
    differ = _differ(m_auto, m_man)
    print("parameter gradients that differ between autograd and the manual chain:", differ)
    assert not differ
    # a class at weight 0: its row of the scoring conv gets no gradient
    k0 = 1
    tr0 = train.Trainer(m_zero, loss_params={"class_weights": (1.0, 0.0, 1.0)})
    l0 = tr0.forward_backward(x, uv=uv)
    fc = m_zero.resnet.net.fc
    assert np.isfinite(l0.item()) and l0.item() > 0
    assert (fc.weight.grad[k0] == 0).all() and fc.bias.grad[k0].item() == 0
    for kk in (0, 2):
        assert fc.weight.grad[kk].abs().max().item() > 0 and fc.bias.grad[kk].item() != 0
    assert (tr0.plane_loss[:, k0] == -1).all() and tr0.plane_used.sum(0).tolist() == [B, 0, B]
    with pytest.raises(ops.HkpError, match="dense target"):
        tr0.forward_backward(x, target=torch.zeros(B, K, H, W, dtype=torch.float64, device=cuda_device))


@pytest.mark.parametrize("class_loss", [True, False])
def test_fit_prints_the_class_loss(cuda_device, tmp_path, monkeypatch, capsys, class_loss):
    import train as train_mod
    from torch.utils.data import DataLoader
    from hkp import ops
    from src.dataset import KeypointsDataset, transform
    K, H, W = 3, 64, 96
    assert train_mod.CLASS_LOSS is False and train_mod.LOSS_PARAMS == {}
    _write_split(tmp_path, "train", 2, 71, K, H, W)
    _write_split(tmp_path, "test", 4, 81, K, H, W)
    sets = [KeypointsDataset(str(tmp_path / s / "images"), str(tmp_path / s / "keypoints"), K, H, W, transform,
                             return_uv=True) for s in ("train", "test")]
    train_data, test_data = (DataLoader(s, batch_size=2, shuffle=False) for s in sets)
    model = _r18(cuda_device, K)
    if class_loss:
        monkeypatch.setattr(train_mod, "CLASS_LOSS", True)
        monkeypatch.setattr(train_mod, "LOSS_PARAMS", {"class_weights": (1.0, 0.0, 2.0), "topk": 1})
    monkeypatch.setattr(train_mod, "_bucketer", None)
    monkeypatch.setattr(train_mod, "optimizer", torch.optim.Adam(model.parameters(), lr=1.0e-4, weight_decay=1.0e-4))
    seen, calls = [], []
    real_planes, real_call = ops.heat_loss_planes, ops.call

    def planes(*a, **kw):
        out = real_planes(*a, **kw)
        seen.append(out[2].cpu())
        return out

    monkeypatch.setattr(ops, "heat_loss_planes", planes)
    monkeypatch.setattr(ops, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    capsys.readouterr()
    train_mod.fit(train_data, test_data, model, epochs=1, checkpoint_path=str(tmp_path))
    out = capsys.readouterr().out
    monkeypatch.setattr(ops, "call", real_call)
    lines = [ln.split("\r")[-1] for ln in out.strip().split("\n")]
    print(lines)
    heads = [ln.split(":")[0] for ln in lines]
    if not class_loss:
        assert heads == ["train loss", "test loss"], lines                        # the reference's lines only
        assert not seen and "hkp_heat_loss_planes" not in calls and calls.count("hkp_heat_loss") == 3
        return
    assert heads == ["train loss", "train class loss", "test loss", "test class loss"], lines
    assert calls.count("hkp_heat_loss_planes") == 3 and len(seen) == 3

    def means(batches):
        pl = torch.cat(batches)
        on = pl >= 0
        s, c = torch.where(on, pl, torch.zeros_like(pl)).sum(0), on.sum(0)
        return [float(a) / int(b) if int(b) else NAN for a, b in zip(s, c)]

    for line, want in ((lines[1], means(seen[:1])), (lines[3], means(seen[1:]))):
        got = [float(v) for v in line.split(":")[1].split()]
        print(line, want)
        assert len(got) == K and np.isnan(got[1]) and np.isnan(want[1])          # class 1 is never labelled
        for a, b in ((got[0], want[0]), (got[2], want[2])):
            assert a > 0 and abs(a - b) <= 4 * 2.0 ** -53 * b
