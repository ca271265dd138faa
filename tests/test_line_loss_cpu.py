"""hkp_heat_loss_lines without a GPU: the float64 reference of tests/_line_loss_ref.py against
the planes and masks references on point labels and against central differences; every
rejection from the C entry up to Trainer(loss_params={"lines": ...}); the new signatures; and
the top-k precondition of the GPU tests' inputs."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import _line_loss_ref as llref
import _lines_ref as lref
import _masks_ref as mref
import _planes_ref as pref

KINDS = [("bce", 2.0), ("mse", 2.0), ("qfl", 2.0), ("qfl", 1.5)]
NAN = float("nan")


def _as_lines(pts):
    return torch.cat([pts[..., 0:2], pts[..., 0:2], pts[..., 2:3]], -1)


def _point_case():
    """Point labels [2,4,3,3] with an absent plane, unpacked slots and junk in empty ones."""
    shape = (2, 4, 3, 9, 11)
    n, k, m, H, W = shape
    g = torch.Generator().manual_seed(3)
    pts = torch.rand(n, k, m, 3, generator=g) * torch.tensor([W + 4.0, H + 4.0, 1.0]) - torch.tensor([2.0, 2.0, 0.0])
    pts[..., 2] = (pts[..., 2] > 0.3).float()
    pts[0, 1, :, 2] = 0.0                                # an absent plane
    pts[1, 2, 0] = torch.tensor([NAN, NAN, -1.0])        # junk in an empty slot
    pts[1, 3, :, 2] = torch.tensor([0.0, 1.0, 1.0])
    p = torch.rand(n, k, H, W, generator=g) * 0.98 + 0.01
    w = torch.rand(n, k, generator=g) + 0.5
    w[0, 2], w[1, 0] = 0.0, NAN
    return shape, p, pts, w


@pytest.mark.parametrize("norm", ["elements", "instances"])
@pytest.mark.parametrize("absent", ["zero", "ignore"])
def test_reference_on_point_labels_is_the_planes_and_masks_reference(absent, norm):
    shape, p, pts, w = _point_case()
    n, k, m, H, W = shape
    lines = _as_lines(pts)
    assert torch.equal(llref.present(lines), (pts[..., 2] > 0).sum(-1))
    y = llref.target(lines.numpy(), H, W, 2.0)
    assert ((y >= 0) & (y <= 1)).all() and (y[0, 1] == 0).all()
    mask = mref.seeded_mask(shape)
    for kind, beta in KINDS:
        for weights in (None, w):
            for topk in (None, 1, 2, k):
                a = llref.line_loss_ref(p, y, lines, None, kind, absent, norm, beta, weights, topk)
                b = pref.planes_ref(p, y, pts, kind, absent, norm, beta, weights, topk)
                assert a["loss"] == b["loss"] and torch.equal(a["dheat"], b["dheat"]) and torch.equal(a["S"], b["S"])
                assert torch.equal(a["used"], b["used"]) and torch.equal(a["plane_loss"], b["plane_loss"])
                assert a["elements"] == b["elements"]
                a = llref.line_loss_ref(p, y, lines, mask, kind, absent, norm, beta, weights, topk)
                b = mref.masked_ref(p, y, pts, mask, kind, absent, norm, beta, weights, topk)
                assert a["loss"] == b["loss"] and torch.equal(a["dheat"], b["dheat"]) and torch.equal(a["S"], b["S"])
                assert torch.equal(a["used"], b["used"]) and torch.equal(a["plane_loss"], b["plane_loss"])
                assert torch.equal(a["plane_pixels"], b["plane_pixels"]) and a["elements"] == b["elements"]
                assert not a["used"][n - 1].any()                          # the image at 0xFF


def _line_case():
    """One small true line plane next to a point plane and an empty one."""
    H, W = 7, 9
    lines = np.stack([lref.fill([lref.seg(1.0, 1.5, 7.0, 5.0), lref.seg(6.0, 0.0, 6.0, 3.0)], 3),
                      lref.fill([lref.seg(4.0, 3.0, 4.0, 3.0)], 3),
                      lref.fill([], 3, junk=(NAN, NAN, NAN, NAN, 0.0))]).reshape(1, 3, 3, 5)
    g = torch.Generator().manual_seed(5)
    p = torch.rand(1, 3, H, W, generator=g) * 0.9 + 0.05
    mask = (torch.rand(1, H, W, generator=g) < 0.3).to(torch.uint8) * 3
    return lines, p, mask, llref.target(lines, H, W, 2.0)


@pytest.mark.parametrize("kind,beta", KINDS)
def test_reference_gradient_against_central_differences(kind, beta):
    lines, p, mask, y = _line_case()
    assert llref.present(lines).tolist() == [[2, 1, 0]]
    assert 0 < float(y[0, 0].min()) and float(y[0, 0].max()) > 0.9 and (y[0, 2] == 0).all()
    w = torch.tensor([[1.5, 0.5, 2.0]])
    h = 1e-3
    for norm in ("elements", "instances"):
        for m in (None, mask):
            ref = llref.line_loss_ref(p, y, lines, m, kind, "ignore", norm, beta, w)
            assert ref["used"].tolist() == [[True, True, False]]
            assert ref["D"] == (3.0 if norm == "instances" else float(ref["elements"]))
            assert (ref["dheat"][0, 2] == 0).all() and ((ref["dheat"] == 0) | ref["keep"]).all()
            for (c, yy, xx) in ((0, 1, 2), (0, 3, 4), (0, 6, 8), (1, 3, 4), (1, 0, 0), (2, 2, 2)):
                hi, lo = p.clone(), p.clone()
                hi[0, c, yy, xx] += h
                lo[0, c, yy, xx] -= h
                num = (llref.line_loss_ref(hi, y, lines, m, kind, "ignore", norm, beta, w)["loss"]
                       - llref.line_loss_ref(lo, y, lines, m, kind, "ignore", norm, beta, w)["loss"]) / \
                    (float(hi[0, c, yy, xx]) - float(lo[0, c, yy, xx]))
                got = float(ref["dheat"][0, c, yy, xx])
                if not (ref["keep"][0, c, yy, xx] and ref["used"][0, c]):
                    assert got == 0.0 and num == 0.0
                else:
                    assert abs(got - num) <= 2e-3 * abs(num) + 1e-12, (kind, norm, c, got, num)


def test_reference_rules_restated():
    """Eligibility, the divisors, plane_loss and the ranking with its ties, on hand values."""
    pres = torch.tensor([[12, 0, 1]])
    npix = torch.tensor([[10, 10, 0]])
    assert llref.eligible(pres, "zero", None, npix).tolist() == [[True, True, False]]
    assert llref.eligible(pres, "ignore", None, npix).tolist() == [[True, False, False]]
    assert llref.eligible(pres, "zero", torch.tensor([[0.0, NAN, 1.0]]), npix).tolist() == [[False, False, False]]
    used = torch.tensor([[True, True, False]])
    assert llref.divisor(pres, npix, used, "instances") == 12.0          # a polyline of 12 pieces counts 12
    assert llref.divisor(pres, npix, used, "elements") == 20.0
    assert llref.divisor(pres, npix, ~used, "elements") == float("inf")
    assert llref.divisor(pres * 0, npix, used, "instances") == 1.0
    S = torch.tensor([[2.0, 2.0, 5.0, NAN]], dtype=torch.float64)
    el = torch.tensor([[True, True, True, True]])
    n4 = torch.tensor([[4, 4, 100, 4]])
    assert llref.select(S, n4, None, el, 1, False).tolist() == [[False, False, False, True]]      # NaN leads
    assert llref.select(S, n4, None, el, 2, False).tolist() == [[False, False, True, True]]
    assert llref.select(S, n4, None, el, 3, False).tolist() == [[True, False, True, True]]        # a tie: the lower class
    assert llref.select(S, n4, None, el, 2, True).tolist() == [[True, False, False, True]]        # means, not sums
    assert llref.select(S, n4, None, el & (S == S), 5, False).tolist() == [[True, True, True, False]]


@pytest.mark.parametrize("shape", llref.TOPK_SHAPES)
def test_topk_precondition_of_the_gpu_inputs(shape):
    """The GPU top-k tests compare a selection: on their inputs (the same tensors) no two
    neighbouring ranks are closer than the planes tests' 8e-4, relative."""
    assert llref.TOPK_SHAPES == mref.TOPK_SHAPES and llref.TOPK_MIN_GAP == 8e-4
    n, k, m, H, W = shape
    for absent in ("zero", "ignore"):
        p, lines, mask = llref.topk_case(shape, absent)
        assert lines.shape == (n, k, m + 2, 5) and (llref.present(lines)[:, 1] == 2).all()
        y = llref.target(lines.numpy(), H, W, 8.0)
        for kind in ("bce", "mse"):
            for w in (None, mref.topk_weights(shape)):
                for mk in (None, mask):
                    ref = llref.line_loss_ref(p, y, lines, mk, kind, absent, "elements", 2.0, w)
                    gap = llref.rank_gap(ref["S"], ref["plane_pixels"], w, ref["eligible"], mk is not None)
                    print("%s %s %s weights %s mask %s: smallest relative rank gap %.3e"
                          % (shape, absent, kind, w is not None, mk is not None, gap))
                    assert gap >= llref.TOPK_MIN_GAP


# ------------------------------------------------------------------------- rejections ----

def test_c_entry_rejects_from_host_records_and_leaves_outputs_alone():
    from hkp import _lib
    L = _lib.lib()
    for name in ("hkp_heat_loss_lines", "hkp_heat_loss_lines_workspace"):
        assert hasattr(L, name) and name in _lib.SIGNATURES
    assert L.hkp_heat_loss_lines_workspace(2, 3, 5, 7) == L.hkp_heat_loss_masked_workspace(2, 3, 5, 7)
    assert L.hkp_heat_loss_lines_workspace(0, 3, 5, 7) == -1 and L.hkp_heat_loss_lines_workspace(2, 3, 5, -1) == -1
    n, k, s, H, W = 2, 3, 4, 5, 6
    heat = np.full((n, k, H, W), 0.5, np.float32)
    lines = np.zeros((n, k, s, 5), np.float32)
    weights = np.ones((n, k), np.float32)
    mask = np.zeros((n, H, W), np.uint8)
    loss, dheat = np.full((1,), 7.0), np.full((n, k, H, W), 7.0, np.float32)
    plane_loss, used, pixels = np.full((n, k), 7.0), np.full((n, k), 7, np.int32), np.full((n, k), 7, np.int32)
    ws = np.full((L.hkp_heat_loss_lines_workspace(n, k, H, W) // 8,), 7.0)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    good = dict(n=n, k=k, s=s, H=H, W=W, kind=_lib.HKP_LOSS_BCE, absent=0, norm=0, beta=2.0, topk=0, heat=P(heat),
                lines=P(lines), weights=P(weights), mask=P(mask), sigma=8.0, loss=P(loss), ws=P(ws))
    bad = [(dict(n=0), "bad sizes"), (dict(n=-1), "bad sizes"), (dict(k=0), "bad sizes"), (dict(H=0), "bad sizes"),
           (dict(W=-3), "bad sizes"), (dict(H=1 << 15, W=(1 << 15) + 1), "bad sizes"), (dict(H=1 << 30, W=2), "bad sizes"),
           (dict(n=1 << 20, k=1 << 5, mask=None), "bad sizes"),
           (dict(s=0), "outside 1..128"), (dict(s=129), "outside 1..128"), (dict(s=-1), "outside 1..128"),
           (dict(sigma=0.0), "sigma"), (dict(sigma=-1.0), "sigma"), (dict(sigma=NAN), "sigma"),
           (dict(sigma=float("inf")), "sigma"),
           (dict(heat=None), "null tensor"), (dict(lines=None), "null tensor"), (dict(loss=None), "null tensor"),
           (dict(ws=None), "null tensor"),
           (dict(kind=3), "bad loss kind"), (dict(kind=-1), "bad loss kind"), (dict(absent=2), "bad absent mode"),
           (dict(absent=-1), "bad absent mode"), (dict(norm=2), "bad norm mode"), (dict(norm=-1), "bad norm mode"),
           (dict(kind=_lib.HKP_LOSS_QFL, beta=0.5), r"outside \[1, 8\]"),
           (dict(kind=_lib.HKP_LOSS_QFL, beta=8.5), r"outside \[1, 8\]"),
           (dict(kind=_lib.HKP_LOSS_QFL, beta=NAN), r"outside \[1, 8\]"),
           (dict(topk=-1), "topk"), (dict(topk=4), "topk"), (dict(n=1, k=65, topk=2, mask=None), "topk"),
           (dict(n=1, k=9), "a mask byte holds 8"), (dict(n=1, k=64), "a mask byte holds 8")]
    for b, what in bad:
        a = dict(good, **b)
        with pytest.raises(_lib.HkpError, match=what):
            _lib.call("hkp_heat_loss_lines", a["n"], a["k"], a["s"], a["H"], a["W"], a["kind"], a["absent"], a["norm"],
                      a["beta"], a["topk"], a["heat"], a["lines"], a["weights"], a["mask"], a["sigma"], a["loss"],
                      P(dheat), P(plane_loss), P(used), P(pixels), a["ws"], None)
        assert L.hkp_last_error().decode().startswith("hkp_heat_loss_lines"), b
    # beta is read by the quality focal kind alone
    assert (loss == 7).all() and (dheat == 7).all() and (plane_loss == 7).all() and (used == 7).all()
    assert (pixels == 7).all() and (ws == 7).all()


def test_python_rejections_before_a_tensor_is_touched():
    """Every tensor here is on the CPU: the argument errors come first, on shapes and numbers
    alone; what passes them is refused for its device, and nothing is computed."""
    from hkp import ops
    from hkp.autograd import line_heatmap_loss
    E = ops.HkpError
    heat, lines = torch.rand(2, 3, 4, 8), torch.zeros(2, 3, 5, 5)
    good_mask = torch.zeros(2, 4, 8, dtype=torch.uint8)
    cases = [(dict(kind="huber"), "unknown kind"), (dict(norm="pixels"), "unknown norm"),
             (dict(absent="skip"), "unknown absent"),
             (dict(kind="qfl", beta=0.5), "beta"), (dict(kind="qfl", beta=NAN), "beta"), (dict(kind="qfl", beta="x"), "beta"),
             (dict(sigma=0.0), "sigma"), (dict(sigma=-2.0), "sigma"), (dict(sigma=NAN), "sigma"),
             (dict(sigma=float("inf")), "sigma"),
             (dict(weights=[1.0] * 6), "weights must be a float32 tensor"), (dict(weights=torch.ones(3, 2)), "weights must be"),
             (dict(weights=torch.ones(2, 3).double()), "weights must be"),
             (dict(topk=0), "topk"), (dict(topk=4), "topk"), (dict(topk=1.0), "topk"), (dict(topk=True), "topk"),
             (dict(mask=good_mask.int()), "mask must be uint8"), (dict(mask=good_mask[0]), "mask must be uint8"),
             (dict(mask=good_mask.numpy()), "mask must be a uint8 tensor"),
             (dict(mask=torch.zeros(2, 8, 4, dtype=torch.uint8)), r"mask must be uint8 \[2,4,8\]"),
             (dict(mask=torch.zeros(2, 8, 4, dtype=torch.uint8).transpose(1, 2)), "mask must be contiguous"),
             (dict(lines=None), "expected a tensor"), (dict(lines=torch.zeros(2, 3, 5)), r"\[N,K,S,5\]"),
             (dict(lines=torch.zeros(2, 3, 5, 3)), r"\[N,K,S,5\]"), (dict(lines=torch.zeros(2, 3, 0, 5)), "1 <= S"),
             (dict(lines=torch.zeros(2, 3, 129, 5)), "1 <= S"),
             (dict(lines=torch.zeros(2, 2, 5, 5)), "not go with"), (dict(lines=torch.zeros(1, 3, 5, 5)), "not go with"),
             (dict(), "on the GPU"), (dict(mask=good_mask, weights=torch.ones(2, 3), topk=2, kind="qfl"), "on the GPU")]
    for fn, who in ((lambda **kw: ops.heat_loss_lines(heat, kw.pop("lines", lines), **kw), "heat_loss_lines"),
                    (lambda **kw: line_heatmap_loss(heat, kw.pop("lines", lines), **kw), "line_heatmap_loss")):
        for kw, msg in cases:
            if "sigma" in kw and who == "line_heatmap_loss":
                msg = "sigma|on the GPU"                 # sigma is ops.heat_loss_lines' to check: the device comes first
            with pytest.raises(E, match=msg):
                fn(**dict(kw))
    with pytest.raises(E, match="lines .* does not go with heat"):
        ops.heat_loss_lines(heat, torch.zeros(2, 3, 5, 5, device="meta"))
    wide = torch.rand(1, 9, 4, 8)
    for fn in (ops.heat_loss_lines, line_heatmap_loss):
        with pytest.raises(E, match="8 class bits, heat has K = 9"):
            fn(wide, torch.zeros(1, 9, 2, 5), mask=good_mask[:1])
        with pytest.raises(E, match="at most 64 with topk"):
            fn(torch.rand(1, 65, 4, 8), torch.zeros(1, 65, 2, 5), topk=2)
    # line_heatmap_loss's own: heat, and pts with the lines
    pts = torch.zeros(2, 3, 2, 3)
    for kw, msg in ((dict(pts=torch.zeros(2, 3, 2)), r"pts must be \[N,K,M,3\]"), (dict(pts=torch.zeros(2, 2, 2, 3)), "pts must be"),
                    (dict(pts=[0.0]), "pts must be"), (dict(pts=torch.zeros(2, 3, 124, 3)), "at most 128 slots"),
                    (dict(pts=pts), "on the GPU"), (dict(pts=pts, return_planes=True), "on the GPU")):
        with pytest.raises(E, match=msg):
            line_heatmap_loss(heat, lines, **kw)
    with pytest.raises(E, match=r"heat must be a tensor \[N,K,H,W\]"):
        line_heatmap_loss(heat[0], lines)


def test_trainer_lines_route_rejections_before_the_forward():
    from hkp import ops, train
    from src.model import KeypointsGauss
    import config
    assert config.LOSS_PARAMS == {} and train.LINES_ROUTES == ("dense", "walk")
    model = KeypointsGauss(3, backbone="resnet18", pretrained=False)
    assert train.Trainer(model).lines_route == "dense"
    assert train.Trainer(model, loss_params={"lines": "dense"}).lines_route == "dense"
    for bad in ("Walk", "registers", None, 1, True):
        with pytest.raises(ValueError, match="lines"):
            train.Trainer(model, loss_params={"lines": bad})
    with pytest.raises(ValueError, match="loss_params may hold"):
        train.Trainer(model, loss_params={"line": "walk"})
    E = ops.HkpError
    x = torch.zeros(1, 3, 32, 32)
    lines, pts = torch.zeros(1, 3, 4, 5), torch.zeros(1, 3, 2, 3)
    walk = {"lines": "walk"}
    tr = train.Trainer(model, loss_params=walk)
    assert tr.lines_route == "walk" and "lines" not in tr.loss_params
    with pytest.raises(E, match="not with uv or target"):
        tr.step(x, uv=torch.zeros(1, 3, 2), lines=lines)
    with pytest.raises(E, match="not with uv or target"):
        tr.forward_backward(x, target=torch.zeros(1, 3, 32, 32, dtype=torch.float64), lines=lines)
    with pytest.raises(E, match="weights must be a float32 tensor"):
        tr.step(x, lines=lines, weights=[1.0, 1.0, 1.0])
    with pytest.raises(E, match="mask must be uint8"):
        tr.step(x, lines=lines, mask=torch.zeros(1, 32, 32))
    with pytest.raises(E, match=r"\[N,K,S,5\]"):
        tr.step(x, lines=torch.zeros(1, 3, 4, 4))
    with pytest.raises(E, match="do not go with"):
        tr.step(x, pts=pts, lines=torch.zeros(1, 2, 4, 5))
    tr9 = train.Trainer(KeypointsGauss(9, backbone="resnet18", pretrained=False), loss_params=walk)
    with pytest.raises(E, match="8 class bits"):
        tr9.step(x, lines=torch.zeros(1, 9, 4, 5), mask=torch.zeros(1, 32, 32, dtype=torch.uint8))
    # what the dense route refuses passes the walk's checks: the device is next
    for kw, step in ((dict(loss="qfl", loss_params=dict(walk, beta=1.5, norm="instances")), dict(lines=lines)),
                     (dict(absent="ignore", loss_params=dict(walk, class_weights=[1.0, 0.5, 2.0], topk=2)),
                      dict(pts=pts, lines=lines)),
                     (dict(loss_params=walk), dict(lines=lines, weights=torch.ones(1, 3),
                                                   mask=torch.zeros(1, 32, 32, dtype=torch.uint8)))):
        with pytest.raises(E, match="on the GPU"):
            train.Trainer(model, **kw).step(x, **step)
    with pytest.raises(E, match="tags need pts"):
        train.Trainer(model, tags={"classes": (0, 1)}, loss_params=walk).step(x, lines=lines)
    # the key changes nothing for a step without lines, and nothing under "dense"
    with pytest.raises(E, match="not supported with lines"):
        train.Trainer(model, loss_params={"lines": "dense", "topk": 2}).step(x, pts=pts, lines=lines)
    with pytest.raises(E, match="'bce' or 'mse'"):
        train.Trainer(model, loss="qfl", loss_params={"lines": "dense"}).step(x, lines=lines)


def test_new_signatures_and_defaults():
    from hkp import ops
    from hkp.autograd import heatmap_loss, line_heatmap_loss
    from hkp.train import Trainer
    sig = inspect.signature(ops.heat_loss_lines).parameters
    assert [(n, p.default) for n, p in sig.items()] == [
        ("heat", inspect.Parameter.empty), ("lines", inspect.Parameter.empty), ("sigma", 8.0), ("kind", "bce"),
        ("absent", "zero"), ("want_grad", True), ("beta", 2.0), ("norm", "elements"), ("weights", None), ("topk", None),
        ("mask", None)]
    assert [n for n, p in sig.items() if p.kind is inspect.Parameter.KEYWORD_ONLY] == ["beta", "norm", "weights", "topk",
                                                                                        "mask"]
    sig = inspect.signature(line_heatmap_loss).parameters
    assert [(n, p.default) for n, p in sig.items()] == [
        ("heat", inspect.Parameter.empty), ("lines", inspect.Parameter.empty), ("sigma", 8.0), ("kind", "bce"),
        ("absent", "zero"), ("pts", None), ("beta", 2.0), ("norm", "elements"), ("weights", None), ("topk", None),
        ("mask", None), ("return_planes", False)]
    assert [n for n, p in sig.items() if p.kind is inspect.Parameter.KEYWORD_ONLY] == [
        "pts", "beta", "norm", "weights", "topk", "mask", "return_planes"]
    for f in (Trainer.step, Trainer.forward_backward, heatmap_loss):        # unchanged
        params = inspect.signature(f).parameters
        assert list(params)[-1] == "lines" and params["lines"].default is None
