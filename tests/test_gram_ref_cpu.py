"""tests/_gram_ref.py checked on the CPU: its Gram moments and its BN statistics
against a brute-force per-pixel float64 computation (Y = A W^T, population mean and
variance), the integer bounds that make the GPU comparison bit-exact, and the
branch of gram_plan each shape of the table is named for."""
import numpy as np
import pytest
import torch

import _bn_ref
import _gram_ref as ref
from _gram_ref import f32, f64


def _dyadic_weight(k, c, seed):
    """A hand-built packed weight: fp16 integers in [-4, 4] and per-channel powers of
    two 2^-3 .. 2^-14 as inverse scales."""
    g = torch.Generator().manual_seed(seed)
    w16 = torch.randint(-4, 5, (k, 1, 1, c), generator=g).half()
    inv = torch.tensor([2.0 ** -(3 + i % 12) for i in range(k)], dtype=torch.float32)
    return w16, inv


@pytest.mark.parametrize("m,c,k", [(64, 64, 16), (37, 128, 24), (1, 64, 8), (200, 192, 40)])
def test_references_are_the_output_statistics(m, c, k):
    a = ref.int_activation(m, c, seed=m + c)
    assert a.dtype == torch.float16 and set(a.unique().tolist()) <= {0.0, 1.0, 2.0, 3.0}
    mu, E = ref.gram_exact(a, chunk=16)
    a64 = a.double().numpy()
    assert np.array_equal(mu.numpy(), a64.sum(0) / m)
    assert np.array_equal(E.numpy(), (a64.T @ a64) / m) and np.array_equal(E.numpy(), E.numpy().T)
    w16, inv = _dyadic_weight(k, c, 3)
    gamma, beta = _bn_ref.rand(k, seed=1) * 0.3 + 1, _bn_ref.rand(k, seed=2)
    rm, rv = _bn_ref.rand(k, seed=3), _bn_ref.rand(k, seed=4).abs() + 0.5
    got = ref.bn_from_gram_exact(mu, E, w16, inv, m, gamma, beta, 0.1, 1e-5, rm, rv)
    # brute force: the conv output itself, pixel by pixel
    w = w16.reshape(k, c).double().numpy() * inv.double().numpy()[:, None]
    y = a64 @ w.T
    mean, var = y.mean(0), y.var(0)
    scale = (np.abs(w) @ a64.max(0)) ** 2 + 1e-300          # the size of the terms that cancel in var
    assert np.allclose(got["mean"], mean, rtol=1e-13, atol=0)
    assert (np.abs(got["var"] - var) <= 1e-12 * scale).all()
    inv_std = 1.0 / np.sqrt(var + f64(f32(1e-5)))
    assert np.allclose(got["mi"][k:].numpy(), inv_std, rtol=2e-7) and np.array_equal(got["mi"][:k].numpy(), mean.astype(f32))
    assert torch.equal(got["ss"], _bn_ref.ss_from_mi(got["mi"], gamma, beta))
    mom = f64(f32(0.1))
    unb = var * m / (m - 1) if m > 1 else var
    assert np.allclose(got["rm"].numpy(), mom * mean + (1 - mom) * rm.double().numpy(), rtol=2e-7, atol=1e-9)
    assert np.allclose(got["rv"].numpy(), mom * unb + (1 - mom) * rv.double().numpy(), rtol=2e-7, atol=1e-9)
    none = ref.bn_from_gram_exact(mu, E, w16, inv, m, None, None)
    assert none["rm"] is None and torch.equal(none["ss"][:k], none["mi"][k:])


def test_clamp_and_zero_rows():
    """A constant input channel gives variance exactly 0; second moments perturbed
    downward give a negative difference, clamped: both 1 / sqrt(eps), never NaN."""
    c, k = 64, 4
    a = ref.int_activation(64, c, seed=9)
    a[:, 0], a[:, 1] = 2, 3
    mu, E = ref.gram_exact(a)
    E[1, 1] -= 2.0 ** -10
    w16, inv = _dyadic_weight(k, c, 5)
    w16[0], w16[1], w16[2] = 0, 0, 0
    w16[0, 0, 0, 0], w16[1, 0, 0, 1] = 3, -2
    got = ref.bn_from_gram_exact(mu, E, w16, inv, 64, None, None)
    assert got["var"][0] == 0 and got["var"][1] == 0 and got["var"][2] == 0 and got["var"][3] > 0
    assert got["mean"][2] == 0 and got["mean"][0] == 6 * 2.0 ** -3 and got["mean"][1] == -6 * 2.0 ** -4
    want = f32(1.0 / np.sqrt(f64(f32(1e-5))))
    assert (got["mi"][k:k + 3].numpy() == want).all() and torch.isfinite(got["ss"]).all()


def test_integer_bounds_hold_for_every_shape():
    for m, c in ref.GRAM_SHAPES:
        p = ref.plan(m, c)
        assert p.rows % 32 == 0 and 32 <= p.rows <= ref.MAX_SPLIT_ROWS
        assert 9 * p.rows < 2 ** 24 and 3 * p.rows < 2 ** 24          # fp32 inside a split
        assert 9 * m < 2 ** 53                                        # fp64 across the splits
        assert 1 <= p.last <= p.rows and (p.splits - 1) * p.rows + p.last == m
    a = ref.int_activation(2048, 64, seed=1)                          # the helper asserts its own bounds
    assert a.shape == (2048, 64) and a.max() == 3 and a.min() == 0
    # different per row and per channel
    assert len({tuple(r) for r in a[:64].tolist()}) == 64 and len({tuple(r) for r in a.T[:64].tolist()}) == 64
    # the hand-built moments of the bn_from_gram tests: C <= 2048, |w| <= 4 * 2^e, 64 E <= 9 * 64
    assert 2048 * 2048 * 9 * 64 * 16 < 2 ** 53
    # the integer conv output: <= 64 non-zeros of |w| <= 4 on activations <= 3
    w = ref.int_weight(8, 256, seed=2)
    assert w.shape == (8, 1, 1, 256) and (w.reshape(8, 256) != 0).sum(1).max() <= 64
    assert (w.reshape(8, 256).abs().sum(1) * 3).max() <= 2048


BRANCH = {
    (1, 64): dict(tc=64, nb=1, tiles=1, rows=32, splits=1, variant=1, last=1),
    (31, 64): dict(rows=32, splits=1, last=31),
    (32, 64): dict(rows=32, splits=1, last=32),
    (33, 64): dict(rows=32, splits=2, last=1),
    (2016, 64): dict(tc=64, rows=32, splits=63, variant=1, last=32),
    (2017, 64): dict(tc=64, rows=32, splits=64, variant=4, last=1),
    (2048, 64): dict(tc=64, rows=32, splits=64, variant=4, last=32),
    (97, 320): dict(tc=64, nb=5, tiles=15, rows=32, splits=4, variant=1, last=1),
    (2700, 192): dict(tc=64, nb=3, tiles=6, rows=32, splits=85, variant=4, last=12),
    (2700, 384): dict(tc=128, nb=3, tiles=6, rows=32, splits=85, variant=4, last=12),
    (300, 1024): dict(tc=128, nb=8, tiles=36, rows=32, splits=10, variant=1, last=12),
    (130, 2048): dict(tc=128, nb=16, tiles=136, rows=64, splits=3, variant=1, last=2),
    (49153, 2048): dict(tc=128, nb=16, tiles=136, rows=16384, splits=4, variant=1, last=1),
}


def test_plan_puts_every_shape_in_its_branch():
    assert set(BRANCH) == set(ref.GRAM_SHAPES)
    for (m, c), want in BRANCH.items():
        p = ref.plan(m, c)
        for key, v in want.items():
            assert getattr(p, key) == v, ((m, c), key, getattr(p, key), v)
        assert p.ws_bytes == p.splits * p.tiles * p.tc ** 2 * 4 + p.splits * c * 4 + 256
    # 49153 is the smallest m whose uncapped split length (m over 512 // 136 = 3 splits) passes the cap
    assert 512 // 136 == 3 and (49152 + 2) // 3 == 16384 and (49153 + 2) // 3 > ref.MAX_SPLIT_ROWS
    assert ref.plan(49152, 2048).rows == 16384 and ref.plan(49152, 2048).splits == 3
    # the chain and real-valued shapes
    assert ref.plan(4096, 64).splits == 128 and ref.plan(30000, 256).rows == 192


@pytest.mark.parametrize("nb", [1, 2, 3, 5, 8, 16])
def test_tile_decode_enumerates_the_upper_triangle(nb):
    tiles = [ref.tile_of(t, nb) for t in range(nb * (nb + 1) // 2)]
    assert tiles == [(i, j) for i in range(nb) for j in range(i, nb)]
