"""hkp_heat_loss_lines on the GPU: bit for bit against the dense chain (hkp_line_target, then
hkp_heat_loss) and, on point labels, against hkp_heat_loss_planes / hkp_heat_loss_masked;
against the float64 reference of tests/_line_loss_ref.py on true line planes (weights, masks,
empty planes, top-k); and the layers above (ops, autograd, Trainer's "walk" route).

The line planes are those of tests/test_gpu_lines.py (imported): horizontal, vertical,
diagonal and zero-length segments, segments across tile borders, partly outside and far
outside, empty planes with flags 0, -1 and NaN over NaN coordinates.  The shapes are
_line_loss_ref.SHAPES.  Each figure is printed before it is asserted (pytest -s)."""
import ctypes

import numpy as np
import pytest
import torch

import _line_loss_ref as llref
import _lines_ref as lref
import _masks_ref as mref
from test_gpu_focal import _labels, _loss_bound, _plus_zero, _within_one_ulp
from test_gpu_instances import SHAPES as POINT_SHAPES
from test_gpu_instances import _heat, _same_bits
from test_gpu_lines import HW_, SCENES3, _batches, _case, _grads, _r18, _spy
from test_gpu_planes import _bits64

pytestmark = pytest.mark.gpu

NAN = float("nan")
SHAPES = llref.SHAPES
SIGMAS = (8.0, 0.75)
ABSENT = ["zero", "ignore"]
NORMS = ["elements", "instances"]
KINDS = [("bce", 2.0), ("mse", 2.0), ("qfl", 2.0), ("qfl", 1.5)]


def _lines_of(shape):
    return torch.from_numpy(np.array(_case(shape)[0]))


def _ref_target(shape, sigma):
    """The restated target (fp32 values as float64) from the case's cached d2."""
    t = lref.target64(_case(shape)[2], sigma)
    return torch.from_numpy(t.astype(np.float32).astype(np.float64))


def _own_target(shape, ld, sigma):
    """The kernel's own dense target on the CPU, after it is held within one fp32 ulp of the
    restated one: what the reference's terms are taken against (the device's expf may differ
    from the float64 exp in the last bit; tests/test_gpu_lines.py does the same)."""
    from hkp import ops
    n, k, s, H, W = shape
    own = ops.line_target(ld, H, W, sigma)[0].cpu()
    want = _ref_target(shape, sigma)
    ulp = np.spacing(np.abs(want.numpy()).astype(np.float32)).astype(np.float64)
    err = np.abs(own.numpy() - want.numpy()) / ulp
    print("%s sigma %g: target worst %.3f ulp from the restatement" % (shape, sigma, err.max()))
    assert (err <= 1.0).all()
    return own


def _close(what, got, want, total, factor=1.0):
    err, bound = abs(got - want), factor * _loss_bound(total, want)
    print("%s: loss %.17g ref %.17g err %.3e bound %.3e" % (what, got, want, err, bound))
    assert np.isfinite(got) and err <= bound, (what, err, bound)


def _planes_close(what, got, want, pixels, factor=1.0):
    """plane_loss: -1 in the same places, the others within the sum bound of the plane's pixels."""
    got, want = got.cpu(), want.cpu()
    print("%s: plane_loss worst error %.3e" % (what, (got - want).abs().max().item()))
    assert torch.equal(got == -1, want == -1)
    assert ((got - want).abs() <= factor * (pixels.cpu().double() + 16) * 2.0 ** -53 * want.abs()).all()


def _all_equal(what, a, b):
    """loss, dheat, plane_loss, plane_used and plane_pixels (when both have it), bit for bit."""
    assert np.array_equal(_bits64(a[0]), _bits64(b[0])), what + ": loss"
    if a[1] is not None or b[1] is not None:
        _same_bits(what, a[1], b[1])
    assert np.array_equal(_bits64(a[2]), _bits64(b[2])), what + ": plane_loss"
    assert torch.equal(a[3], b[3]), what + ": plane_used"
    if a[4] is not None and b[4] is not None:
        assert torch.equal(a[4], b[4]), what + ": plane_pixels"


def _against(what, got, ref, keep=None):
    """One call's five outputs against a line_loss_ref dict."""
    loss, dheat, plane_loss, plane_used, plane_pixels = got
    _within_one_ulp(what, dheat, ref["dheat"])
    g = dheat.cpu()
    assert _plus_zero(g[~ref["used"]])
    if keep is not None:
        assert _plus_zero(g[~keep])
        assert torch.equal(plane_pixels.cpu().long(), ref["plane_pixels"])
    else:
        assert plane_pixels is None
    assert torch.equal(plane_used.cpu().bool(), ref["used"])
    _planes_close(what, plane_loss, ref["plane_loss"], ref["plane_pixels"])
    _close(what, loss.item(), ref["loss"], ref["elements"])
    assert torch.isfinite(plane_loss).all()


# ------------------------------------------------------- 1. bit equalities: the dense chain ----

@pytest.mark.parametrize("shape", SHAPES)
def test_dheat_has_the_bits_of_the_dense_chain(cuda_device, shape):
    from hkp import ops
    n, k, s, H, W = shape
    pd, ld = llref.heat(shape).to(cuda_device), _lines_of(shape).to(cuda_device)
    with torch.cuda.device(cuda_device):
        for sigma in SIGMAS:
            target = ops.line_target(ld, H, W, sigma)[0]
            for kind in ("bce", "mse"):
                want_loss, want = ops.heat_loss(pd, target, None, sigma, kind)
                loss, dheat, plane_loss, plane_used, plane_pixels = ops.heat_loss_lines(pd, ld, sigma, kind)
                what = "dense chain %s %s sigma %g" % (shape, kind, sigma)
                _same_bits(what, dheat, want)
                _close(what, loss.item(), want_loss.item(), n * k * H * W, 2.0)
                assert plane_pixels is None and plane_used.dtype == torch.int32 and (plane_used == 1).all()
                assert plane_loss.dtype == torch.float64 and (plane_loss >= 0).all()


# ------------------------------------------------------ 2. bit equalities: the point planes ----

@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("absent", ABSENT)
@pytest.mark.parametrize("shape", POINT_SHAPES)
def test_point_planes_have_the_bits_of_the_planes_and_masked_entries(cuda_device, shape, absent, norm):
    """lines = from_points(pts) at M = 1: the same fp32 operations for the target, so dheat and
    the integer outputs are equal; the sums differ in their order alone."""
    from hkp import lines as L
    from hkp import ops
    n, k, m, H, W = shape
    pd = _heat(shape).to(cuda_device)
    ptsd = _labels(shape, absent)[:, :, :1].contiguous().to(cuda_device)
    ld = L.from_points(ptsd)
    assert ld.shape == (n, k, 1, 5)
    md = mref.seeded_mask(shape).to(cuda_device)
    with torch.cuda.device(cuda_device):
        for kind, beta in KINDS:
            what = "points %s %s %g %s %s" % (shape, kind, beta, absent, norm)
            a = ops.heat_loss_planes(pd, ptsd, 8.0, kind, absent, beta=beta, norm=norm)
            b = ops.heat_loss_lines(pd, ld, 8.0, kind, absent, beta=beta, norm=norm)
            _same_bits(what, b[1], a[1])
            assert torch.equal(b[3], a[3]) and b[4] is None
            _close(what, b[0].item(), a[0].item(), n * k * H * W, 2.0)
            _planes_close(what, b[2], a[2], torch.full((n, k), H * W), 2.0)
            a = ops.heat_loss_masked(pd, ptsd, md, 8.0, kind, absent, beta=beta, norm=norm)
            b = ops.heat_loss_lines(pd, ld, 8.0, kind, absent, beta=beta, norm=norm, mask=md)
            _same_bits(what + " masked", b[1], a[1])
            assert torch.equal(b[3], a[3]) and torch.equal(b[4], a[4]) and b[4].dtype == torch.int32
            _close(what + " masked", b[0].item(), a[0].item(), int((a[4] * a[3]).sum()), 2.0)
            _planes_close(what + " masked", b[2], a[2], a[4], 2.0)


# ------------------------------------------------------------- 3. against the reference ----

@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("absent", ABSENT)
@pytest.mark.parametrize("shape", SHAPES)
def test_line_planes_against_the_reference(cuda_device, shape, absent, norm):
    from hkp import ops
    n, k, s, H, W = shape
    lines = _lines_of(shape)
    p = llref.heat(shape)
    sat = p.clone()                                                    # saturated: exactly 0 and 1
    sat.view(-1)[0::3] = 0.0
    sat.view(-1)[1::5] = 1.0
    mask = llref.seeded_mask(shape)
    keep = llref.keep_of(mask, n, k, H, W)
    pd, sd, ld, md = p.to(cuda_device), sat.to(cuda_device), lines.to(cuda_device), mask.to(cuda_device)
    with torch.cuda.device(cuda_device):
        for sigma in SIGMAS:
            y = _own_target(shape, ld, sigma)
            for kind, beta in KINDS:
                for heat, hd, tag in ((p, pd, ""), (sat, sd, " saturated")):
                    if tag and sigma != SIGMAS[0]:
                        continue
                    what = "%s %s %g %s %s sigma %g%s" % (shape, kind, beta, absent, norm, sigma, tag)
                    ref = llref.line_loss_ref(heat, y, lines, None, kind, absent, norm, beta)
                    got = ops.heat_loss_lines(hd, ld, sigma, kind, absent, beta=beta, norm=norm)
                    _against(what, got, ref)
                    ref = llref.line_loss_ref(heat, y, lines, mask, kind, absent, norm, beta)
                    got = ops.heat_loss_lines(hd, ld, sigma, kind, absent, beta=beta, norm=norm, mask=md)
                    _against(what + " masked", got, ref, keep)
                    assert np.isfinite(got[0].item()) and torch.isfinite(got[1]).all()


# ---------------------------------------------------------------------------- 4. weights ----

@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3], SHAPES[4]])
def test_weights(cuda_device, shape):
    from hkp import ops
    n, k, s, H, W = shape
    lines, p, mask = _lines_of(shape), llref.heat(shape), llref.seeded_mask(shape)
    keep = llref.keep_of(mask, n, k, H, W)
    w = llref.weights(shape)
    # not labelled: weights 0, NaN and -1, as many of them as leave a plane in the loss
    bad = list(zip([0, n * k - 1, 1], [0.0, NAN, -1.0]))[:max(1, min(3, n * k - 1))]
    off = torch.zeros(n * k, dtype=torch.bool)
    wbad = w.clone()
    for at, v in bad:
        off[at], wbad.view(-1)[at] = True, v
    off = off.view(n, k)
    assert not off.all()
    # NaN under the planes that are not labelled and under every masked pixel
    dirty = torch.where(keep & ~off.view(n, k, 1, 1), p, torch.full_like(p, NAN))
    dirty_planes = torch.where(~off.view(n, k, 1, 1).expand_as(p), p, torch.full_like(p, NAN))
    pd, ld, md = p.to(cuda_device), lines.to(cuda_device), mask.to(cuda_device)
    ones = torch.ones(n, k, device=cuda_device)
    with torch.cuda.device(cuda_device):
        y = _own_target(shape, ld, 8.0)
        for kind, beta in KINDS:
            for absent in ABSENT:
                for norm in NORMS:
                    kw = dict(beta=beta, norm=norm)
                    what = "weights %s %s %g %s %s" % (shape, kind, beta, absent, norm)
                    for m_cpu, m_dev in ((None, None), (mask, md)):
                        _all_equal(what + " of one", ops.heat_loss_lines(pd, ld, 8.0, kind, absent, weights=ones, mask=m_dev, **kw),
                                   ops.heat_loss_lines(pd, ld, 8.0, kind, absent, mask=m_dev, **kw))
                        for wt in (w, wbad):
                            ref = llref.line_loss_ref(p, y, lines, m_cpu, kind, absent, norm, beta, wt)
                            got = ops.heat_loss_lines(pd, ld, 8.0, kind, absent, weights=wt.to(cuda_device), mask=m_dev, **kw)
                            _against(what + (" masked" if m_cpu is not None else ""), got, ref,
                                     keep if m_cpu is not None else None)
                        assert _plus_zero(got[1].cpu()[off]) and (got[2].cpu()[off] == -1).all()
                        assert not got[3].cpu()[off].any()
                        hd = (dirty if m_cpu is not None else dirty_planes).to(cuda_device)
                        again = ops.heat_loss_lines(hd, ld, 8.0, kind, absent, weights=wbad.to(cuda_device), mask=m_dev, **kw)
                        _all_equal(what + " with NaN where nothing is read", again, got)


# ------------------------------------------------------------------------------ 5. masks ----

@pytest.mark.parametrize("shape", SHAPES)
def test_all_zero_and_all_ones_masks(cuda_device, shape):
    from hkp import ops
    n, k, s, H, W = shape
    pd, ld = llref.heat(shape).to(cuda_device), _lines_of(shape).to(cuda_device)
    zero = torch.zeros(n, H, W, dtype=torch.uint8, device=cuda_device)
    full = torch.full((n, H, W), 0xFF, dtype=torch.uint8, device=cuda_device)
    nanp = torch.full_like(pd, NAN)
    with torch.cuda.device(cuda_device):
        for kind, beta in KINDS:
            for absent in ABSENT:
                for norm in NORMS:
                    for topk in (None, 1):
                        kw = dict(beta=beta, norm=norm, topk=topk)
                        a = ops.heat_loss_lines(pd, ld, 8.0, kind, absent, **kw)
                        b = ops.heat_loss_lines(pd, ld, 8.0, kind, absent, mask=zero, **kw)
                        _all_equal("zero mask %s %s %s %s topk %s" % (shape, kind, absent, norm, topk), b, a)
                        el = (b[2] != -1).int()
                        assert a[4] is None and b[4].dtype == torch.int32 and torch.equal(b[4], el * (H * W))
                        loss, dheat, pl, pu, px = ops.heat_loss_lines(nanp, ld, 8.0, kind, absent, mask=full, **kw)
                        assert loss.item() == 0.0 and _plus_zero(dheat) and (pl == -1).all() and not pu.any() and not px.any()


# ----------------------------------------------------------------------- 6. empty planes ----

def test_empty_planes(cuda_device):
    from hkp import ops
    shape = SHAPES[1]
    n, k, s, H, W = shape
    lines, kinds, _ = _case(shape)
    assert 2 in kinds                                                  # an empty plane among the others
    lines = torch.from_numpy(np.array(lines))
    empty = ~(lines[..., 4] > 0).any(-1)
    assert empty.any() and not empty.all()
    none = lines.clone()
    none[..., 4] = torch.tensor([0.0, -1.0, NAN, 0.0])                 # no present slot in the batch
    p = llref.heat(shape)
    pd = p.to(cuda_device)
    with torch.cuda.device(cuda_device):
        y = _own_target(shape, lines.to(cuda_device), 8.0)
        for kind, beta in KINDS:
            for norm in NORMS:
                # "ignore": the empty plane leaves the divisor
                got = ops.heat_loss_lines(pd, lines.to(cuda_device), 8.0, kind, "ignore", beta=beta, norm=norm)
                ref = llref.line_loss_ref(p, y, lines, None, kind, "ignore", norm, beta)
                assert torch.equal(got[3].cpu().bool(), ~empty) and torch.equal(ref["used"], ~empty)
                assert ref["D"] == (float(H * W * int((~empty).sum())) if norm == "elements"
                                    else float(int(llref.present(lines).sum())))
                _against("empty plane ignored %s %s" % (kind, norm), got, ref)
                assert _plus_zero(got[1].cpu()[empty]) and (got[2].cpu()[empty] == -1).all()
                # nothing present anywhere
                loss, dheat, pl, pu, px = ops.heat_loss_lines(pd, none.to(cuda_device), 8.0, kind, "ignore", beta=beta,
                                                              norm=norm)
                assert loss.item() == 0.0 and _plus_zero(dheat) and (pl == -1).all() and not pu.any()
                got = ops.heat_loss_lines(pd, none.to(cuda_device), 8.0, kind, "zero", beta=beta, norm=norm)
                ref = llref.line_loss_ref(p, torch.zeros_like(y), none, None, kind, "zero", norm, beta)
                assert ref["D"] == (1.0 if norm == "instances" else float(n * k * H * W)) and ref["used"].all()
                _against("nothing present, zero %s %s" % (kind, norm), got, ref)
                assert np.isfinite(got[0].item()) and got[0].item() > 0


# ------------------------------------------------------------------------------ 7. top-k ----

@pytest.mark.parametrize("kind", ["bce", "mse"])
@pytest.mark.parametrize("shape", llref.TOPK_SHAPES)
def test_topk_against_the_reference(cuda_device, shape, kind):
    from hkp import ops
    n, k, m, H, W = shape
    with torch.cuda.device(cuda_device):
        for absent in ABSENT:
            p, lines, mask = llref.topk_case(shape, absent)
            pd, ld = p.to(cuda_device), lines.to(cuda_device)
            y = ops.line_target(ld, H, W, 8.0)[0].cpu()
            for mk in (None, mask):
                md = None if mk is None else mk.to(cuda_device)
                keep = None if mk is None else llref.keep_of(mk, n, k, H, W)
                for w in (None, mref.topk_weights(shape)):
                    wd = None if w is None else w.to(cuda_device)
                    base = llref.line_loss_ref(p, y, lines, mk, kind, absent, "elements", 2.0, w)
                    gap = llref.rank_gap(base["S"], base["plane_pixels"], w, base["eligible"], mk is not None)
                    print("top-k %s %s %s weights %s mask %s: smallest relative rank gap %.3e"
                          % (shape, kind, absent, w is not None, mk is not None, gap))
                    assert gap >= llref.TOPK_MIN_GAP                   # test_line_loss_cpu.py pins it too
                    for norm in NORMS:
                        plain = ops.heat_loss_lines(pd, ld, 8.0, kind, absent, norm=norm, weights=wd, mask=md)
                        for T in (1, 2, k):
                            ref = llref.line_loss_ref(p, y, lines, mk, kind, absent, norm, 2.0, w, T)
                            what = "top-%d %s %s %s %s weights %s mask %s" % (T, shape, kind, absent, norm, w is not None,
                                                                            mk is not None)
                            got = ops.heat_loss_lines(pd, ld, 8.0, kind, absent, norm=norm, weights=wd, topk=T, mask=md)
                            used = ref["used"]
                            assert (used.sum(1) == torch.minimum(ref["eligible"].sum(1), torch.tensor(T))).all()
                            _against(what, got, ref, keep)
                            assert np.array_equal(_bits64(got[2]), _bits64(plain[2]))   # not counted: the value stays
                            sel = used.float() * (1.0 if w is None else w)
                            as_w = ops.heat_loss_lines(pd, ld, 8.0, kind, absent, norm=norm, weights=sel.to(cuda_device),
                                                       mask=md)
                            _same_bits(what + " vs the selection as weights", got[1], as_w[1])
                            if T == k:
                                _all_equal(what + " vs topk=None", got, plain)


def test_topk_tie_goes_to_the_lower_class(cuda_device):
    from hkp import ops
    shape = (1, 4, 3, 35, 66)
    n, k, s, H, W = shape
    one = torch.from_numpy(np.array(_case(SHAPES[4])[0]))[0, 0, :3]    # a true line plane
    lines = one.view(1, 1, 3, 5).repeat(1, k, 1, 1).contiguous()
    plane = llref.heat((1, 1, 1, H, W))
    p = plane.repeat(1, k, 1, 1).contiguous()
    p[0, 3] = p[0, 3] * 0.5                                            # class 3 differs, 0..2 are identical
    with torch.cuda.device(cuda_device):
        for kind, beta in KINDS:
            for T in (1, 2, 3):
                loss, dheat, pl, pu, px = ops.heat_loss_lines(p.to(cuda_device), lines.to(cuda_device), 8.0, kind, beta=beta,
                                                              topk=T)
                pl = pl.cpu()
                assert pl[0, 0] == pl[0, 1] == pl[0, 2] and pl[0, 3] != pl[0, 0]
                first = [3] if pl[0, 3] > pl[0, 0] else []
                want = (first + [0, 1, 2])[:T]
                assert sorted(pu.cpu()[0].nonzero().view(-1).tolist()) == sorted(want), (kind, T)


# ------------------------------------------------------------- 8. every way of asking ----

@pytest.mark.parametrize("topk", [None, 2])
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[4], SHAPES[5]])
def test_second_run_and_missing_outputs_give_the_same_bits(cuda_device, shape, topk):
    from hkp import _lib, ops
    n, k, s, H, W = shape
    topk = None if topk is None else min(topk, k)
    pd, ld = llref.heat(shape).to(cuda_device), _lines_of(shape).to(cuda_device)
    wd, md = llref.weights(shape).to(cuda_device), llref.seeded_mask(shape).to(cuda_device)
    P = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731
    with torch.cuda.device(cuda_device):
        for kind, beta in KINDS:
            for mask in (None, md):
                kw = dict(beta=beta, weights=wd, topk=topk, mask=mask)
                a = ops.heat_loss_lines(pd, ld, 8.0, kind, "ignore", **kw)
                b = ops.heat_loss_lines(pd, ld, 8.0, kind, "ignore", **kw)
                _all_equal("second run", b, a)
                c = ops.heat_loss_lines(pd, ld, 8.0, kind, "ignore", want_grad=False, **kw)
                assert c[1] is None
                _all_equal("without dheat", c, (a[0], None, a[2], a[3], a[4]))
                ws = torch.empty(_lib.lib().hkp_heat_loss_lines_workspace(n, k, H, W) // 8, device=cuda_device,
                                 dtype=torch.float64)
                loss = torch.full((), NAN, device=cuda_device, dtype=torch.float64)
                dheat = torch.full_like(pd, 7.0)
                _lib.call("hkp_heat_loss_lines", n, k, s, H, W, {"bce": 0, "mse": 1, "qfl": 2}[kind], 1, 0, beta, topk or 0,
                          P(pd), P(ld), P(wd), None if mask is None else P(mask), 8.0, P(loss), P(dheat), None, None, None,
                          P(ws), ops._stream())
                assert np.array_equal(_bits64(a[0]), _bits64(loss))
                _same_bits("without the plane outputs", dheat, a[1])


@pytest.mark.parametrize("shape", llref.VEC_SHAPES)
def test_views_off_their_alignment(cuda_device, shape):
    """The 16-byte shapes with heat and dheat one element off a 16-byte boundary (the scalar
    path) and the mask one byte off a 4-byte boundary (byte loads): the same bits, and the
    guard values around dheat stay."""
    from hkp import _lib, ops
    n, k, s, H, W = shape
    assert W % 4 == 0
    numel = n * k * H * W
    pd, ld = llref.heat(shape).to(cuda_device), _lines_of(shape).to(cuda_device)
    md = llref.seeded_mask(shape).to(cuda_device)
    wd = llref.weights(shape).to(cuda_device)
    P = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731
    with torch.cuda.device(cuda_device):
        assert pd.data_ptr() % 16 == 0 and md.data_ptr() % 4 == 0
        hb = torch.full((numel + 8,), 0.5, device=cuda_device)
        hv = hb[1:1 + numel].view(n, k, H, W)
        hv.copy_(pd)
        mb = torch.full((n * H * W + 8,), 0xFF, dtype=torch.uint8, device=cuda_device)
        mv = mb[1:1 + n * H * W].view(n, H, W)
        mv.copy_(md)
        assert hv.data_ptr() % 16 == 4 and mv.data_ptr() % 4 == 1
        ws = torch.empty(_lib.lib().hkp_heat_loss_lines_workspace(n, k, H, W) // 8, device=cuda_device,
                         dtype=torch.float64)
        for kind, beta in KINDS:
            for topk in (None, 1):
                for heat, mask, doff in ((hv, md, 1), (pd, mv, 0), (hv, mv, 1), (pd, md, 3), (hv, None, 1)):
                    what = "off alignment %s %s topk %s heat %d mask %s dheat %d" % (
                        shape, kind, topk, heat.data_ptr() % 16, None if mask is None else mask.data_ptr() % 4, doff)
                    want = ops.heat_loss_lines(pd, ld, 8.0, kind, "ignore", beta=beta, weights=wd, topk=topk,
                                               mask=None if mask is None else md)
                    db = torch.full((numel + 8,), 7.0, device=cuda_device)
                    dv = db[doff:doff + numel].view(n, k, H, W)
                    loss = torch.full((), NAN, device=cuda_device, dtype=torch.float64)
                    pl = torch.empty(n, k, device=cuda_device, dtype=torch.float64)
                    pu = torch.empty(n, k, device=cuda_device, dtype=torch.int32)
                    px = torch.empty(n, k, device=cuda_device, dtype=torch.int32)
                    _lib.call("hkp_heat_loss_lines", n, k, s, H, W, {"bce": 0, "mse": 1, "qfl": 2}[kind], 1, 0, beta,
                              topk or 0, P(heat), P(ld), P(wd), None if mask is None else P(mask), 8.0, P(loss), P(dv),
                              P(pl), P(pu), None if mask is None else P(px), P(ws), ops._stream())
                    _all_equal(what, (loss, dv, pl, pu, None if mask is None else px), want)
                    assert (db[:doff] == 7).all() and (db[doff + numel:] == 7).all()
        assert (hb[0] == 0.5) and (mb[0] == 0xFF)


# ------------------------------------------------------------------ 9. the layers above ----

def _manual(m, img, lab, kind, **kw):
    """The forward, ops.heat_loss_lines and the hand-written backward, call by call."""
    from hkp import net, ops
    trace = net.Trace(m.policy)
    hm, _, _ = net.keypoints_forward(m.resnet.net, img, m.num_keypoints, heat=True, trace=trace)
    out = ops.heat_loss_lines(hm, lab, 8.0, kind, **kw)
    grads = net.keypoints_backward(m.resnet.net, trace, out[1], net.Grads())
    return out, [grads[p].clone() for p in m.parameters()], hm


def _equal_grads(what, got, want, m):
    differ = [tuple(p.shape) for p, g, w in zip(m.parameters(), got, want) if not torch.equal(g, w)]
    print("%s: parameter gradients that differ: %s" % (what, differ))
    assert not differ


def test_trainer_walk_route_is_the_manual_chain(cuda_device):
    from hkp import lines as L
    from hkp.autograd import line_heatmap_loss
    from hkp.train import Trainer
    m = _r18(cuda_device, 3)
    with torch.cuda.device(cuda_device):
        img, pts, lines = next(iter(_batches(cuda_device, SCENES3, 33, 4, 4, fixed=True)))
        assert (lines[:, 2, :, 4] > 0).any()
        lab = L.concat(L.from_points(pts), lines)
        for kind in ("bce", "mse"):
            tr = Trainer(m, loss=kind, loss_params={"lines": "walk"})
            loss = tr.forward_backward(img, pts=pts, lines=lines)
            got = _grads(m)
            out, want, hm = _manual(m, img, lab, kind)
            assert np.array_equal(_bits64(loss), _bits64(out[0])) and np.isfinite(loss.item()) and loss.item() > 0
            _equal_grads("walk step vs manual chain, " + kind, got, want, m)
            assert torch.equal(tr.plane_loss, out[2]) and torch.equal(tr.plane_used, out[3]) and tr.plane_pixels is None
            # the autograd function: through the model, and on the heatmaps alone
            for p in m.parameters():
                p.grad = None
            la = line_heatmap_loss(m(img), lines, kind=kind, pts=pts)
            assert la.requires_grad and la.dtype == torch.float64
            la.backward()
            assert np.array_equal(_bits64(la.detach()), _bits64(out[0]))
            _equal_grads("line_heatmap_loss vs manual chain, " + kind, _grads(m), want, m)
            hm2 = hm.detach().clone().requires_grad_(True)
            l2, pl2, pu2 = line_heatmap_loss(hm2, lines, kind=kind, pts=pts, return_planes=True)
            l2.backward()
            assert torch.equal(hm2.grad, out[1]) and torch.equal(pl2, out[2]) and not pl2.requires_grad
            # the dense route trains the same: its dheat has the same bits
            Trainer(m, loss=kind).forward_backward(img, pts=pts, lines=lines)
            _equal_grads("walk vs dense, " + kind, _grads(m), want, m)
        # lines alone
        tr = Trainer(m, loss_params={"lines": "walk"})
        loss = tr.step(img, lines=lines)
        assert np.isfinite(loss.item())


def test_trainer_walk_route_with_qfl_mask_and_topk(cuda_device):
    from hkp import lines as L
    from hkp.train import Trainer
    m = _r18(cuda_device, 3)
    B, K = 4, 3
    with torch.cuda.device(cuda_device):
        img, pts, lines = next(iter(_batches(cuda_device, SCENES3, 33, 4, 4, fixed=True)))
        lab = L.concat(L.from_points(pts), lines)
        mask = llref.seeded_mask((B, K, 1) + HW_).to(cuda_device)
        mask[B - 1] = mask[0]
        mask |= 2                                                      # class 1 is masked everywhere
        w = torch.rand(B, K, generator=torch.Generator().manual_seed(2)).to(cuda_device) + 0.5
        cw = [1.0, 2.0, 0.5]
        tr = Trainer(m, loss="qfl", absent="ignore",
                     loss_params={"lines": "walk", "beta": 2.0, "norm": "instances", "topk": 2, "class_weights": cw})
        loss = tr.forward_backward(img, pts=pts, lines=lines, weights=w, mask=mask)
        got = _grads(m)
        wk = (torch.tensor(cw, device=cuda_device)[None, :] * w).contiguous()
        out, want, _ = _manual(m, img, lab, "qfl", absent="ignore", beta=2.0, norm="instances", topk=2, weights=wk,
                               mask=mask)
        print("walk qfl + mask + topk loss %.17g, manual %.17g" % (loss.item(), out[0].item()))
        assert np.array_equal(_bits64(loss), _bits64(out[0])) and np.isfinite(loss.item()) and loss.item() > 0
        _equal_grads("walk qfl + mask + topk", got, want, m)
        assert all(torch.isfinite(g).all() for g in got)
        assert torch.equal(tr.plane_loss, out[2]) and torch.equal(tr.plane_used, out[3])
        assert torch.equal(tr.plane_pixels, out[4]) and tr.plane_pixels.is_cuda
        assert (tr.plane_pixels[:, 1] == 0).all() and not tr.plane_used[:, 1].any() and tr.plane_used.any()
        # the class masked everywhere: its row of the scoring conv gets exactly nothing
        fc = m.resnet.net.fc
        gw, gb = [g for p, g in zip(m.parameters(), got) if p is fc.weight][0], \
            [g for p, g in zip(m.parameters(), got) if p is fc.bias][0]
        assert (gw[1] == 0).all() and gb[1].item() == 0
        assert gw[0].abs().max().item() > 0 or gw[2].abs().max().item() > 0
        tr.forward_backward(img, pts=pts, lines=lines)
        assert tr.plane_pixels is None and tr.plane_loss is not None


def test_library_calls_of_both_routes(cuda_device, monkeypatch):
    """"walk" replaces hkp_line_target, hkp_heat_loss by one hkp_heat_loss_lines and moves
    nothing else; under the default every call is what it was."""
    from hkp.train import Trainer
    m = _r18(cuda_device, 3)
    with torch.cuda.device(cuda_device):
        img, pts, lines = next(iter(_batches(cuda_device, SCENES3, 33, 4, 4, fixed=True)))
        Trainer(m).forward_backward(img, pts=pts, lines=lines)             # packs the weights: not compared
        calls = _spy(monkeypatch)
        Trainer(m).forward_backward(img, pts=pts, lines=lines)
        dense = list(calls)
        at = dense.index("hkp_line_target")
        assert dense[at:at + 2] == ["hkp_line_target", "hkp_heat_loss"] and "hkp_heat_loss_lines" not in dense
        assert dense.count("hkp_line_target") == 1 and dense.count("hkp_heat_loss") == 1
        del calls[:]
        Trainer(m, loss_params={"lines": "dense"}).forward_backward(img, pts=pts, lines=lines)
        assert list(calls) == dense
        del calls[:]
        Trainer(m, loss_params={"lines": "walk"}).forward_backward(img, pts=pts, lines=lines)
        walk = [c for c in calls if not c.endswith("_workspace")]
        assert walk == dense[:at] + ["hkp_heat_loss_lines"] + dense[at + 2:]
        del calls[:]
        Trainer(m, loss_params={"lines": "walk"}).forward_backward(img, lines=lines)
        assert [c for c in calls if not c.endswith("_workspace")] == walk
        # a step without lines does not see the key
        del calls[:]
        Trainer(m).forward_backward(img, pts=pts)
        plain = list(calls)
        del calls[:]
        Trainer(m, loss_params={"lines": "walk"}).forward_backward(img, pts=pts)
        assert list(calls) == plain and "hkp_heat_loss_lines" not in plain
