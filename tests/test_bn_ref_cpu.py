"""The restatements of tests/_bn_ref.py checked against torch on the CPU in float64:
what test_gpu_bn.py compares the kernels with must itself be BatchNorm, its
backward, and the stem pool.  float64-level tolerances; 2^-22 relative where a
restatement is fp32 by design."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _bn_ref as ref
from _bn_ref import rand

EPS32 = 2.0 ** -22


def _partials(y, tile_rows):
    """fp32 (sum, M2 about the tile mean) per tile of tile_rows rows of y [M, C]."""
    out = []
    for r0 in range(0, y.shape[0], tile_rows):
        t = y[r0:r0 + tile_rows].double()
        out.append(torch.stack([t.sum(0), ((t - t.mean(0)) ** 2).sum(0)], -1))
    return torch.stack(out).float()


@pytest.mark.parametrize("m,c,rows", [(37, 8, 16), (130, 32, 128), (1, 4, 4), (96, 12, 96)])
def test_finalize_and_apply_are_batch_norm(m, c, rows):
    y = rand(m, c, seed=m) * 2 + 0.7
    gamma, beta = rand(c, seed=1) * 0.3 + 1, rand(c, seed=2)
    rm, rv = rand(c, seed=3), rand(c, seed=4).abs() + 0.5
    fin = ref.finalize(_partials(y, rows), m, rows, gamma, beta, 0.1, 1e-5, rm, rv)
    rm64, rv64 = rm.double(), rv.double()
    if m > 1:
        want = F.batch_norm(y.double().t()[None], rm64, rv64, gamma.double(), beta.double(), True,
                            float(np.float32(0.1)), float(np.float32(1e-5)))[0].t()
        assert torch.allclose(fin["rm"].double(), rm64, rtol=EPS32, atol=1e-7)
        assert torch.allclose(fin["rv"].double(), rv64, rtol=EPS32, atol=1e-7)
    else:    # one row: F.batch_norm refuses it; the statistics are the row and 0
        want = beta.double()[None].expand(1, c)
        assert np.array_equal(fin["m2"], np.zeros(c))
        assert torch.allclose(fin["rv"].double(), (1 - float(np.float32(0.1))) * rv64, rtol=EPS32, atol=0)
    # the partials are fp32-rounded (2^-24 relative each) and mean/invstd are rounded to fp32
    mean64 = y.double().mean(0)
    assert np.allclose(fin["mean"], mean64.numpy(), rtol=1e-6, atol=1e-6)
    # fp32 mean and invstd, then two fp32 roundings: each an ulp of |y| or |mean|, times |alpha|
    tol = 8 * EPS32 * max(1.0, y.abs().max().item() * 2) * max(1.0, fin["ss"][:c].abs().max().item())
    for relu in (False, True):
        got = ref.apply(y, fin["ss"], relu=relu)
        w = F.relu(want) if relu else want
        assert (got.double() - w).abs().max() <= tol
    # the fp32 tail on the restatement's own mean/invstd
    assert torch.equal(ref.ss_from_mi(fin["mi"], gamma, beta), fin["ss"])


def test_finalize_tile_sizes_agree():
    """The merge is exact in float64 up to its own rounding: any tiling of the same
    rows gives the same statistics (fp32 partials: 1e-6)."""
    y = rand(301, 8, seed=5) * 3 + 1.5
    outs = [ref.finalize(_partials(y, r), 301, r, None, None) for r in (4, 96, 128, 301)]
    for o in outs[1:]:
        assert np.allclose(o["mean"], outs[0]["mean"], rtol=1e-6, atol=1e-7)
        assert np.allclose(o["m2"], outs[0]["m2"], rtol=1e-6)
    assert np.allclose(outs[0]["m2"] / 301, y.double().var(0, unbiased=False).numpy(), rtol=1e-6)


def test_apply_residual_forms_and_nan_rule():
    c = 32
    y, res = rand(5, c, seed=6), rand(5, c, seed=7)
    ss, rss = rand(2 * c, seed=8), rand(2 * c, seed=9)
    base = y.double() * ss[:c].double() + ss[c:].double()
    for kw, add in ((dict(res=res), res.double()),
                    (dict(res=res, res_ss=rss), res.double() * rss[:c].double() + rss[c:].double()),
                    (dict(res_split=ref.split(res, 3)), res.double())):
        got = ref.apply(y, ss, relu=True, **kw)
        assert (got.double() - F.relu(base + add)).abs().max() <= 8 * EPS32 * 4
    y[0, 0], y[1, 1], y[2, 2] = float("nan"), float("inf"), -float("inf")
    ss[:3] = ss[:3].abs() + 0.1
    on, off = ref.apply(y, ss, relu=True), ref.apply(y, ss, relu=False)
    assert on[0, 0] == 0 and torch.isnan(off[0, 0])                  # the project's rule, not torch.relu's
    assert on[1, 1] == float("inf") and on[2, 2] == 0 and off[2, 2] == -float("inf")
    h16, o32 = ref.apply_f16(y.half(), ss, res.half(), rss, relu=True)
    assert torch.equal(h16, o32.half()) and o32[0, 0] == 0


@pytest.mark.parametrize("c", [32, 96])
def test_split_definition(c):
    o = rand(7, c, seed=10) * 300
    hi = ref.split(o, 1)
    packed = ref.split(o, 3)
    h2, lo = ref.unsplit(packed)
    assert packed.shape == (7, 2 * c) and torch.equal(h2, hi)
    assert torch.equal(packed[:, :32], hi[:, :32]) and torch.equal(packed[:, 64:96], hi[:, 32:64])
    back = hi.double() + lo.double()
    assert ((back - o.double()).abs() <= EPS32 * o.double().abs()).all()


def test_eval_params():
    c = 9
    gamma, beta, rm, rv = rand(c, seed=11), rand(c, seed=12), rand(c, seed=13), rand(c, seed=14).abs() + 0.1
    ss, mi = ref.eval_params(gamma, beta, rm, rv)
    x = rand(4, c, seed=15)
    want = F.batch_norm(x.double(), rm.double(), rv.double(), gamma.double(), beta.double(), False, 0.0,
                        float(np.float32(1e-5)))
    assert (ref.apply(x, ss, relu=False).double() - want).abs().max() <= 8 * EPS32 * 8
    ss1, _ = ref.eval_params(None, None, rm, rv)
    assert torch.equal(ss1[:c], mi[c:])


@pytest.mark.parametrize("m,c,mode", [(65, 8, 1), (130, 4, 2), (63, 32, 0), (1, 4, 0)])
def test_backward_chain_is_autograd(m, c, mode):
    y = (rand(m, c, seed=20) * 2 + 0.3).double().requires_grad_(True)
    gamma = (rand(c, seed=21) * 0.2 + 1).double().requires_grad_(True)
    beta = (rand(c, seed=22) * 0.1).double().requires_grad_(True)
    g = rand(m, c, seed=23)
    y32 = y.detach().float()
    if m > 1:
        z = F.batch_norm(y.t()[None], None, None, gamma, beta, True, 0.1, float(np.float32(1e-5)))[0].t()
        out = F.relu(z) if mode else z
        out.backward(g.double())
    # forward statistics as the forward's finalize leaves them (fp32 mean, invstd)
    fin = ref.finalize(_partials(y32, 64), m, 64, gamma.detach().float(), beta.detach().float())
    mi, ss = fin["mi"], fin["ss"]
    mask = None if mode == 0 else ref.apply(y32, ss, relu=True) if mode == 1 else ss
    dz, sums, sabs, maxima = ref.bwd_tile_sums(g, mask, y32, mi[:c])
    assert sums.shape == ((m + 63) // 64, c, 2) and (np.abs(sums) <= sabs * (1 + 1e-15)).all()
    if mode:      # the two mask forms agree
        other = ss if mode == 1 else ref.apply(y32, ss, relu=True)
        assert torch.equal(ref.bwd_tile_sums(g, other, y32, mi[:c])[0], dz)
    ym = (y32 - mi[:c]).abs()
    assert torch.equal(maxima[:, :, 0].max(0).values, dz.abs().max(0).values)
    assert torch.equal(maxima[:, :, 1].max(0).values, ym.max(0).values)
    co = ref.bwd_coef(torch.from_numpy(sums).float(), maxima, m, mi, gamma.detach().float())
    dy = ref.bwd_apply(dz, y32, mi[:c], co["coef"])
    assert co["bound"] >= dy.abs().max().item()
    assert ref.bwd_bound(co["coef"], co["md"], co["mv"]) == co["bound"]
    assert ref.bwd_coef(torch.from_numpy(sums).float(), None, m, mi, None)["bound"] is None
    if m > 1:
        # fp32 statistics, partials and five fp32 roundings in the apply: 2^-22 of the largest term
        scale = max(1.0, y.grad.abs().max().item(), dz.abs().max().item() * co["coef"][2 * c:].abs().max().item())
        assert (dy.double() - y.grad).abs().max() <= 16 * EPS32 * scale
        assert (co["dgamma"].double() - gamma.grad).abs().max() <= 16 * EPS32 * max(1.0, sabs[:, :, 1].sum(0).max() * 3)
        assert (co["dbeta"].double() - beta.grad).abs().max() <= EPS32 * max(1.0, sabs[:, :, 0].sum(0).max())
    else:         # one row: dz - mean(dz) = 0, y - mean = 0
        assert torch.equal(dy, torch.zeros_like(dy))


def test_pow2_scale():
    for b, want in ((1.0, 2.0 ** 13), (0.75, 2.0 ** 14), (2.0 ** 13, 1.0), (3e-30, 2.0 ** 100), (0.0, 1.0),
                    (float("inf"), 1.0), (float("nan"), 1.0)):
        assert ref.pow2_scale(b) == want, b
    assert 2 ** 13 <= 5.3e-3 * ref.pow2_scale(5.3e-3) < 2 ** 14


@pytest.mark.parametrize("shape", [(2, 9, 11, 4), (1, 8, 6, 8), (1, 1, 1, 4), (1, 2, 5, 4)])
def test_maxpool_and_backward_are_torch(shape):
    n, h, w, c = shape
    y = rand(*shape, seed=30).requires_grad_(True)
    a, b = rand(c, seed=31), rand(c, seed=32) * 0.3
    a[0] = 0.0                                       # a constant channel: ties, first tap wins
    t = (y.double() * a.double() + b.double())
    p = F.max_pool2d(F.relu(t).permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    gp = rand(*p.shape, seed=33)
    (dt,) = torch.autograd.grad(p, t, gp.double())
    out, route = ref.maxpool(y.detach(), torch.cat([a, b]))
    p32 = F.max_pool2d(ref.relu_rule(y.detach() * a + b).permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    assert torch.equal(out, p32)
    assert (out.double() - p).abs().max() <= EPS32 * max(1.0, p.abs().max().item())
    assert route.dtype == torch.uint8 and ((route <= 8) | (route == 255)).all()
    assert torch.equal(route == 255, ~(out > 0))
    dz = ref.maxpool_bwd(gp, route, shape)
    live = a != 0                                    # (ties on the constant channel: torch's choice may differ)
    assert (dz.double()[..., live] - dt[..., live]).abs().max() <= EPS32 * max(1.0, dt.abs().max().item())
    if b[0] <= 0:
        assert torch.equal(dz[..., 0], torch.zeros_like(dz[..., 0]))
    else:         # the whole window's gradient goes to its first valid tap; nothing is lost
        assert abs(dz[..., 0].double().sum().item() - gp[..., 0].double().sum().item()) <= 1e-4


def test_maxpool_nan_never_wins():
    y = rand(1, 5, 5, 4, seed=34)
    y[0, 2, 2, 0] = float("nan")
    y[0, :, :, 1] = float("nan")
    ss = torch.cat([torch.ones(4), torch.zeros(4)])
    out, route = ref.maxpool(y, ss)
    assert not torch.isnan(out).any()
    assert torch.equal(out[..., 1], torch.zeros(1, 3, 3)) and (route[..., 1] == 255).all()
    clean = y.clone()
    clean[0, 2, 2, 0] = 0.0
    o2, r2 = ref.maxpool(clean, ss)
    assert torch.equal(out[..., 0], o2[..., 0]) and torch.equal(route[..., 0], r2[..., 0])
