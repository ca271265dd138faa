"""hkp_heat_loss_planes without a GPU: the float64 reference of tests/_planes_ref.py against
torch's weight= semantics and against hand-written top-k answers, the Python-side
rejections (all before a tensor is touched), the signatures' defaults, the Trainer's and
config's keys, and the C ABI's argument checks (which return before any launch)."""
import ctypes
import inspect

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _instances_ref as iref
import _planes_ref as pref

NAN = float("nan")


def _case():
    n, k, m, H, W = 2, 4, 2, 9, 11
    g = torch.Generator().manual_seed(5)
    p = torch.rand(n, k, H, W, generator=g)
    pts = torch.zeros(n, k, m, 3)
    pts[..., 0] = torch.rand(n, k, m, generator=g) * W
    pts[..., 1] = torch.rand(n, k, m, generator=g) * H
    pts[..., 2] = 1.0
    pts[0, 1, :, 2] = 0.0                                  # an absent plane
    pts[1, 2, 1, 2] = 0.0                                  # one slot of two
    y = torch.from_numpy(iref.gauss_target_multi(pts.numpy(), H, W, 3.0)).double()
    w = torch.rand(n, k, generator=g) * 1.5 + 0.25
    return p, y, pts, w


@pytest.mark.parametrize("norm", ["elements", "instances"])
@pytest.mark.parametrize("absent", ["zero", "ignore"])
def test_positive_weights_are_torchs_weight_argument(absent, norm):
    p, y, pts, w = _case()
    ref = pref.planes_ref(p, y, pts, "bce", absent, norm, weights=w)
    el = pref.eligible(pts, absent, w)
    assert torch.equal(ref["used"], el) and int(el.sum()) == (7 if absent == "ignore" else 8)
    D = float(9 * 11 * int(el.sum())) if norm == "elements" else float(int(((pts[..., 2] > 0).sum(-1) * el).sum()))
    assert ref["D"] == D
    q = p.clone().requires_grad_(True)
    wm = (w * el)[..., None, None].double()                # an absent plane under "ignore": weight 0, finite heat
    want = F.binary_cross_entropy(q.double(), y, weight=wm.expand_as(y), reduction="sum") / D
    want.backward()
    assert abs(ref["loss"] - want.item()) <= 1e-13 * want.item()
    assert np.abs(ref["dheat"].numpy().astype(np.float64) - q.grad.numpy()).max() <= \
        2.0 ** -23 * np.abs(q.grad.numpy()).max()
    assert (ref["dheat"][~el] == 0).all()
    # the per-plane values are the unweighted means
    means = F.binary_cross_entropy(p.double(), y, reduction="none").mean((2, 3))
    assert torch.allclose(ref["plane_loss"][el], means[el], rtol=1e-13, atol=0)
    assert (ref["plane_loss"][~el] == -1).all()


def test_hand_written_topk():
    S = torch.tensor([[4.0, 9.0, 9.0, 1.0],
                      [2.0, 3.0, 5.0, 7.0]], dtype=torch.float64)
    every = torch.ones(2, 4, dtype=torch.bool)
    U = lambda rows: torch.tensor(rows, dtype=torch.bool)                      # noqa: E731
    # a tie: classes 1 and 2 of image 0 both hold 9; the lower class wins
    assert torch.equal(pref.select(S, None, every, 1), U([[0, 1, 0, 0], [0, 0, 0, 1]]))
    assert torch.equal(pref.select(S, None, every, 2), U([[0, 1, 1, 0], [0, 0, 1, 1]]))
    assert torch.equal(pref.select(S, None, every, 3), U([[1, 1, 1, 0], [0, 1, 1, 1]]))
    assert torch.equal(pref.select(S, None, every, 4), every)
    assert torch.equal(pref.select(S, None, every, None), every)
    # weights change the ranking: r = w * S
    w = torch.tensor([[3.0, 1.0, 1.0, 10.0], [1.0, 1.0, 1.0, 0.25]])
    assert torch.equal(pref.select(S, w, every, 2), U([[1, 0, 0, 1], [0, 1, 1, 0]]))
    # fewer eligible planes than T: all of them, and no others
    el = U([[0, 1, 0, 0], [1, 0, 1, 1]])
    assert torch.equal(pref.select(S, None, el, 2), U([[0, 1, 0, 0], [0, 0, 1, 1]]))
    assert torch.equal(pref.select(S, None, el, 3), el)
    # weight 0, negative and NaN: not labelled, whatever their S
    w = torch.tensor([[0.0, -1.0, NAN, 1.0], [1.0, 1.0, 0.0, 1.0]])
    pts = torch.ones(2, 4, 1, 3)
    el = pref.eligible(pts, "zero", w)
    assert torch.equal(el, U([[0, 0, 0, 1], [1, 1, 0, 1]]))
    assert torch.equal(pref.select(S, w, el, 2), U([[0, 0, 0, 1], [0, 1, 0, 1]]))
    assert pref.divisor(pts, 5, 7, pref.select(S, w, el, 2), "elements") == 35.0 * 3
    assert pref.divisor(pts, 5, 7, pref.select(S, w, el, 2), "instances") == 3.0
    assert pref.divisor(pts, 5, 7, torch.zeros(2, 4, dtype=torch.bool), "instances") == 1.0
    # a NaN sum ranks above everything; two NaN go to the lower class
    Sn = torch.tensor([[4.0, NAN, 9.0, NAN]], dtype=torch.float64)
    one = torch.ones(1, 4, dtype=torch.bool)
    assert torch.equal(pref.select(Sn, None, one, 1), U([[0, 1, 0, 0]]))
    assert torch.equal(pref.select(Sn, None, one, 3), U([[0, 1, 1, 1]]))
    assert pref.rank_gap(S, None, every) == 0.0 and abs(pref.rank_gap(S[1:], None, every[1:]) - 2.0 / 7.0) < 1e-15


def test_topk_in_the_reference_zeroes_the_other_planes():
    p, y, pts, w = _case()
    full = pref.planes_ref(p, y, pts, "mse", "zero", "elements", weights=w)
    ref = pref.planes_ref(p, y, pts, "mse", "zero", "elements", weights=w, topk=2)
    assert ref["used"].sum(1).tolist() == [2, 2] and ref["D"] == 9 * 11 * 4.0
    assert torch.equal(ref["plane_loss"], full["plane_loss"])                 # not counted: the value stays
    r = w.double() * ref["S"]
    for b in range(2):
        assert set(torch.nonzero(ref["used"][b]).flatten().tolist()) == set(r[b].topk(2).indices.tolist())
    assert (ref["dheat"][~ref["used"]] == 0).all() and (ref["dheat"][ref["used"]] != 0).any()
    want = (r * ref["used"]).sum().item() / ref["D"]
    assert abs(ref["loss"] - want) <= 1e-14 * want
    # NaN heat in a plane that is not labelled never reaches the result
    w0 = w.clone()
    w0[1, 3] = 0.0
    pn = p.clone()
    pn[1, 3] = NAN
    a = pref.planes_ref(p, y, pts, "bce", "zero", "instances", weights=w0)
    b = pref.planes_ref(pn, y, pts, "bce", "zero", "instances", weights=w0)
    assert np.isfinite(b["loss"]) and a["loss"] == b["loss"] and torch.equal(a["dheat"], b["dheat"])
    assert b["plane_loss"][1, 3] == -1 and not b["used"][1, 3]
    none = pref.planes_ref(pn, y, pts, "bce", "ignore", "elements", weights=torch.zeros(2, 4))
    assert none["loss"] == 0.0 and not none["dheat"].any() and none["D"] == float("inf")


def test_rejections_come_before_any_tensor_is_touched():
    """CPU tensors (or none at all) reach every one of these errors; the last calls show
    that nothing else was wrong."""
    from hkp import autograd as hkp_autograd
    from hkp import ops
    from hkp._lib import HkpError
    heat = torch.rand(2, 3, 5, 7)
    pts = torch.zeros(2, 3, 4, 3)
    uv = torch.zeros(2, 3, 2)
    w = torch.ones(2, 3)
    for fn in (lambda **kw: ops.heat_loss_planes(heat, pts, **kw), lambda **kw: ops.heat_loss_multi(heat, pts, **kw),
               lambda **kw: ops.heat_loss(heat, uv=uv, **kw),
               lambda **kw: hkp_autograd.heatmap_loss(heat, pts=pts, **kw),
               lambda **kw: hkp_autograd.heatmap_loss(heat, uv=uv, **kw)):
        for topk in (0, -1, 2.0, "2", True):
            with pytest.raises(HkpError, match="topk"):
                fn(topk=topk)
        with pytest.raises(HkpError, match="topk 4 outside 1..K"):
            fn(topk=4)
        with pytest.raises(HkpError, match="weights must be"):
            fn(weights=[[1.0] * 3] * 2)
        for bad in (torch.ones(2, 4), torch.ones(3, 2), torch.ones(2, 3, dtype=torch.float64), torch.ones(6),
                    torch.ones(3, 2).t()):
            with pytest.raises(HkpError, match="weights must be"):
                fn(weights=bad)
        with pytest.raises(HkpError, match="unknown kind 'l1'"):
            fn(kind="l1", topk=1)
        with pytest.raises(HkpError, match="unknown norm 'planes'"):
            fn(norm="planes", weights=w)
        with pytest.raises(HkpError, match=r"beta .* outside \[1, 8\]"):
            fn(kind="qfl", beta=0.5, topk=1)
        with pytest.raises(HkpError, match="must be on the GPU"):
            fn(weights=w, topk=3)
    with pytest.raises(HkpError, match="unknown absent 'skip'"):
        ops.heat_loss_planes(heat, pts, absent="skip")
    with pytest.raises(HkpError, match="unknown absent 'skip'"):
        ops.heat_loss_multi(heat, pts, absent="skip", topk=1)
    # K = 65 with top-k
    wide, wide_pts = torch.rand(1, 65, 2, 2), torch.zeros(1, 65, 1, 3)
    with pytest.raises(HkpError, match="at most 64"):
        ops.heat_loss_planes(wide, wide_pts, topk=2)
    with pytest.raises(HkpError, match="must be on the GPU"):
        ops.heat_loss_planes(wide, wide_pts, weights=torch.ones(1, 65))
    # a dense target with either argument
    for kw in ({"weights": w}, {"topk": 1}):
        with pytest.raises(HkpError, match="dense target is not supported"):
            ops.heat_loss(heat, target=heat.double(), **kw)
        with pytest.raises(HkpError, match="dense target is not supported"):
            hkp_autograd.heatmap_loss(heat, target=heat.double(), **kw)
    with pytest.raises(HkpError, match="dense target is not supported"):
        hkp_autograd.heatmap_loss(heat, target=heat.double(), return_planes=True)


def test_signature_defaults():
    import config
    from hkp import autograd as hkp_autograd
    from hkp import ops, train
    ps = inspect.signature(ops.heat_loss_planes).parameters
    assert list(ps) == ["heat", "pts", "sigma", "kind", "absent", "want_grad", "beta", "norm", "weights", "topk"]
    assert [ps[n].default for n in list(ps)[2:]] == [8.0, "bce", "zero", True, 2.0, "elements", None, None]
    for fn in (ops.heat_loss_planes, ops.heat_loss_multi, ops.heat_loss):
        ps = inspect.signature(fn).parameters
        for name in ("beta", "norm", "weights", "topk"):
            assert ps[name].kind is inspect.Parameter.KEYWORD_ONLY, (fn, name)
        assert ps["weights"].default is None and ps["topk"].default is None
    ps = inspect.signature(hkp_autograd.heatmap_loss).parameters
    assert ps["weights"].default is None and ps["topk"].default is None and ps["return_planes"].default is False
    for fn in (train.Trainer.forward_backward, train.Trainer.step):
        assert inspect.signature(fn).parameters["weights"].default is None
    assert config.CLASS_LOSS is False and config.LOSS_PARAMS == {}
    assert ops.TOPK_MAX_K == 64


def test_trainer_accepts_the_new_keys():
    from hkp import ops, train
    from src.model import KeypointsGauss
    m = KeypointsGauss(3, backbone="resnet18", pretrained=False)
    tr = train.Trainer(m, loss_params={"class_weights": (1.0, 0.0, 2.5), "topk": 2})
    assert tr.topk == 2 and tr._class_weights == [1.0, 0.0, 2.5] and tr.loss_params == {}
    assert tr.plane_loss is None and tr.plane_used is None
    tr = train.Trainer(m, loss="qfl", loss_params={"beta": 1.5, "norm": "instances", "topk": 1})
    assert tr.topk == 1 and tr.loss_params == {"beta": 1.5, "norm": "instances"} and tr._class_weights is None
    assert train.Trainer(m).topk is None
    with pytest.raises(ValueError):
        train.Trainer(m, loss_params={"gamma": 2.0})
    with pytest.raises(ValueError):
        train.Trainer(m, loss_params={"class_weights": (1.0, 2.0)})          # K = 3
    with pytest.raises(ops.HkpError, match="topk"):
        train.Trainer(m, loss_params={"topk": 0})


def test_c_abi_rejects_before_any_launch():
    """No pointer here is real: every one of these returns HKP_ERR_BAD_ARG first."""
    from hkp import _lib
    L = _lib.lib()
    assert hasattr(L, "hkp_heat_loss_planes") and "hkp_heat_loss_planes" in _lib.SIGNATURES
    assert L.hkp_heat_loss_planes_workspace(2, 3, 5, 7) >= (1 + 6 * 64 + 6) * 8 + 2 * 6 * 4
    assert L.hkp_heat_loss_planes_workspace(2, 3, 5, 7) % 8 == 0
    assert L.hkp_heat_loss_planes_workspace(0, 3, 5, 7) == -1
    P = ctypes.c_void_p(16)
    ok = dict(n=2, k=3, m=4, kind=_lib.HKP_LOSS_BCE, absent=0, norm=0, beta=2.0, topk=0, heat=P, pts=P, loss=P, ws=P)

    def planes(**kw):
        a = dict(ok, **kw)
        _lib.call("hkp_heat_loss_planes", a["n"], a["k"], a["m"], 5, 7, a["kind"], a["absent"], a["norm"], a["beta"],
                  a["topk"], a["heat"], a["pts"], None, 8.0, a["loss"], None, None, None, a["ws"], None)

    for topk in (-1, 4, 1 << 30):
        with pytest.raises(_lib.HkpError, match="topk"):
            planes(topk=topk)
    with pytest.raises(_lib.HkpError, match="topk"):
        planes(n=1, k=65, topk=2)
    for name in ("heat", "pts", "loss", "ws"):
        with pytest.raises(_lib.HkpError, match="null tensor"):
            planes(**{name: None})
        with pytest.raises(_lib.HkpError, match="null tensor"):
            planes(**{name: None, "topk": 2})
    for beta in (0.5, 8.5, NAN, float("inf")):
        with pytest.raises(_lib.HkpError, match=r"outside \[1, 8\]"):
            planes(kind=_lib.HKP_LOSS_QFL, beta=beta)
    with pytest.raises(_lib.HkpError, match="bad loss kind"):
        planes(kind=3)
    with pytest.raises(_lib.HkpError, match="bad norm mode"):
        planes(norm=2)
    with pytest.raises(_lib.HkpError, match="bad absent mode"):
        planes(absent=-1)
    for m in (0, 17):
        with pytest.raises(_lib.HkpError, match="bad sizes"):
            planes(m=m)
    with pytest.raises(_lib.HkpError, match="bad sizes"):
        planes(n=0)
