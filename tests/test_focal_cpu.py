"""The quality focal loss without a GPU: the float64 reference of tests/_focal_ref.py
checked against finite differences and against the header's closed form, the properties
the decode relies on (the minimum at p == t), and every new argument error."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _focal_ref as fref

BETAS = [1.0, 1.5, 2.0, 4.0]


def _xy(n=400, seed=0):
    """x in [0.05, 0.95], y in [0, 1] with |x - y| >= 0.01: away from the kink of |x - y|
    (beta = 1) and from the ends, where the third derivative grows like 1 / x^3."""
    g = torch.Generator().manual_seed(seed)
    x = 0.05 + 0.9 * torch.rand(n, generator=g, dtype=torch.float64)
    y = torch.rand(n, generator=g, dtype=torch.float64)
    y[::7] = 0.0
    y[3::7] = 1.0
    keep = (x - y).abs() >= 0.01
    assert keep.sum() > n // 2
    return x[keep], y[keep]


@pytest.mark.parametrize("beta", BETAS)
def test_reference_gradient_against_finite_differences(beta):
    x, y = _xy()
    xr = x.clone().requires_grad_(True)
    fref.qfl_terms(xr, y, beta).sum().backward()
    h = 1e-6
    fd = (fref.qfl_terms(x + h, y, beta) - fref.qfl_terms(x - h, y, beta)) / (2 * h)
    # central differences: h^2 f''' / 6 <= 1e-12 * 8000 * 100 / 6 (x >= 0.05; beta = 4: a
    # few more factors of order one) and rounding eps * |f| / h <= 2.2e-16 * 100 / 1e-6
    err = (xr.grad - fd).abs() / (1.0 + fd.abs())
    print("beta %g: worst finite-difference error %.3e" % (beta, err.max().item()))
    assert err.max().item() <= 1e-6
    # and the closed form of include/hulkkp.h, to float64 rounding
    l, g = fref.qfl_formula(x.numpy(), y.numpy(), beta)
    assert np.allclose(fref.qfl_terms(x, y, beta).numpy(), l, rtol=1e-13, atol=0)
    assert np.allclose(xr.grad.numpy(), g, rtol=1e-12, atol=0)


@pytest.mark.parametrize("beta", BETAS)
def test_zero_loss_and_gradient_at_the_target(beta):
    g = torch.Generator().manual_seed(1)
    p = torch.rand(3, 2, 5, 7, generator=g)
    p[0, 0, 0] = 0.0                                     # the clamped logs
    p[0, 0, 1] = 1.0
    loss, grad = fref.qfl_ref(p, p.double(), beta, 17.0)
    assert loss.item() == 0.0 and (grad == 0).all() and torch.isfinite(grad).all()
    l, gg = fref.qfl_formula(p.numpy(), p.numpy(), beta)
    assert (l == 0).all() and (gg == 0).all()


@pytest.mark.parametrize("beta", BETAS)
def test_minimum_is_at_the_target(beta):
    t = torch.linspace(0, 1, 21, dtype=torch.float64)
    at = fref.qfl_terms(t.clone(), t, beta)
    assert (at == 0).all()
    for step in (0.05, -0.05):
        p = t + step
        ok = (p >= 0) & (p <= 1)
        off = fref.qfl_terms(p[ok], t[ok], beta)
        assert ok.sum() == 20 and (off > at[ok]).all(), (beta, step)
        # the gradient points back to the target
        pr = p[ok].clone().requires_grad_(True)
        fref.qfl_terms(pr, t[ok], beta).sum().backward()
        assert (torch.sign(pr.grad) == math.copysign(1.0, step)).all()


def test_divisors():
    pts = torch.zeros(2, 3, 4, 3)
    assert fref.divisor(pts, 5, 7, "zero", "elements") == 2 * 3 * 35
    assert fref.divisor(pts, 5, 7, "ignore", "elements") == float("inf")
    assert fref.divisor(pts, 5, 7, "zero", "instances") == 1.0 == fref.divisor(pts, 5, 7, "ignore", "instances")
    pts[0, 1, 2, 2] = 1.0
    pts[0, 1, 3, 2] = 2.0
    pts[1, 2, 0, 2] = 0.5
    pts[1, 0, 0, 2] = -1.0                               # not present
    pts[1, 0, 1, 2] = float("nan")                       # not present
    assert fref.divisor(pts, 5, 7, "ignore", "elements") == 35 * 2
    assert fref.divisor(pts, 5, 7, "zero", "instances") == 3.0


def test_library_exports_the_call():
    from hkp import _lib, ops
    L = _lib.lib()
    assert hasattr(L, "hkp_heat_loss_multi_ex") and "hkp_heat_loss_multi_ex" in _lib.SIGNATURES
    assert (_lib.HKP_LOSS_BCE, _lib.HKP_LOSS_MSE, _lib.HKP_LOSS_QFL) == (0, 1, 2)
    assert (_lib.HKP_NORM_ELEMENTS, _lib.HKP_NORM_INSTANCES) == (0, 1)
    assert ops.LOSS_KINDS == ("bce", "mse", "qfl") and ops.NORM_MODES == ("elements", "instances")


def test_bad_arguments_raise_through_ops():
    """Names and beta are checked before any tensor is looked at, so CPU tensors reach
    every one of these errors; the last call shows that nothing else was wrong."""
    from hkp import autograd as hkp_autograd
    from hkp import ops
    from hkp._lib import HkpError
    heat = torch.rand(2, 3, 5, 7)
    pts = torch.zeros(2, 3, 4, 3)
    uv = torch.zeros(2, 3, 2)
    with pytest.raises(HkpError, match="unknown kind 'l1'"):
        ops.heat_loss_multi(heat, pts, kind="l1")
    with pytest.raises(HkpError, match="unknown norm 'planes'"):
        ops.heat_loss_multi(heat, pts, kind="qfl", norm="planes")
    with pytest.raises(HkpError, match="unknown norm 'planes'"):
        ops.heat_loss_multi(heat, pts, norm="planes")
    for beta in (0.5, 8.5, -2.0, float("nan"), float("inf")):
        with pytest.raises(HkpError, match=r"beta .* outside \[1, 8\]"):
            ops.heat_loss_multi(heat, pts, kind="qfl", beta=beta)
        with pytest.raises(HkpError, match=r"beta .* outside \[1, 8\]"):
            ops.heat_loss(heat, uv=uv, kind="qfl", beta=beta)
        with pytest.raises(HkpError, match=r"beta .* outside \[1, 8\]"):
            hkp_autograd.heatmap_loss(heat, pts=pts, kind="qfl", beta=beta)
    with pytest.raises(HkpError, match="beta must be a number"):
        ops.heat_loss_multi(heat, pts, kind="qfl", beta="two")
    with pytest.raises(HkpError, match="unknown absent 'skip'"):
        ops.heat_loss_multi(heat, pts, kind="qfl", absent="skip")
    with pytest.raises(HkpError, match="dense target is not supported"):
        ops.heat_loss(heat, target=heat.double(), kind="qfl")
    with pytest.raises(HkpError, match="dense target is not supported"):
        hkp_autograd.heatmap_loss(heat, target=heat.double(), kind="qfl")
    with pytest.raises(HkpError, match="unknown norm 'planes'"):
        ops.heat_loss(heat, uv=uv, kind="qfl", norm="planes")
    with pytest.raises(HkpError, match="needs kind 'qfl' or instance labels"):
        ops.heat_loss(heat, uv=uv, kind="bce", norm="instances")
    # well-formed: the only thing left to object to is where the tensors live
    for beta in (1.0, 2.0, 8.0):
        with pytest.raises(HkpError, match="must be on the GPU"):
            ops.heat_loss_multi(heat, pts, kind="qfl", beta=beta, norm="instances")
    with pytest.raises(HkpError, match="must be on the GPU"):
        ops.heat_loss(heat, uv=uv, kind="qfl")


def test_bad_arguments_raise_in_the_c_abi():
    """hkp_heat_loss_multi_ex rejects before it launches: no pointer here is real."""
    from hkp import _lib
    P = ctypes.c_void_p(16)
    ok = dict(kind=_lib.HKP_LOSS_QFL, absent=0, norm=0, beta=2.0, m=4)

    def ex(**kw):
        a = dict(ok, **kw)
        _lib.call("hkp_heat_loss_multi_ex", 2, 3, a["m"], 5, 7, a["kind"], a["absent"], a["norm"], a["beta"],
                  a.get("heat", P), P, 8.0, P, None, P, None)

    for beta in (0.5, 8.5, -2.0, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(_lib.HkpError, match=r"outside \[1, 8\]"):
            ex(beta=beta)
    with pytest.raises(_lib.HkpError, match="bad loss kind"):
        ex(kind=3)
    with pytest.raises(_lib.HkpError, match="bad loss kind"):
        ex(kind=-1)
    with pytest.raises(_lib.HkpError, match="bad norm mode"):
        ex(norm=2)
    with pytest.raises(_lib.HkpError, match="bad absent mode"):
        ex(absent=2)
    with pytest.raises(_lib.HkpError, match="bad sizes"):
        ex(m=17)
    with pytest.raises(_lib.HkpError, match="null tensor"):
        ex(heat=None)
    # beta is not read for the other kinds, but the norm mode is
    with pytest.raises(_lib.HkpError, match="bad norm mode"):
        ex(kind=_lib.HKP_LOSS_BCE, beta=float("nan"), norm=5)


def test_trainer_and_config_surface():
    import inspect

    import config
    from hkp import autograd as hkp_autograd
    from hkp import ops, train
    assert config.LOSS == "bce" and config.LOSS_PARAMS == {}
    sig = inspect.signature(train.Trainer.__init__)
    assert sig.parameters["loss_params"].default is None
    for fn in (ops.heat_loss, ops.heat_loss_multi):
        ps = inspect.signature(fn).parameters
        assert ps["beta"].default == 2.0 and ps["norm"].default == "elements"
        assert ps["beta"].kind is inspect.Parameter.KEYWORD_ONLY and ps["norm"].kind is inspect.Parameter.KEYWORD_ONLY
    ps = inspect.signature(hkp_autograd.heatmap_loss).parameters
    assert ps["beta"].default == 2.0 and ps["norm"].default == "elements"
