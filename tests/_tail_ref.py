"""CPU references for the tail of the network — the heatmap head, its backward,
the loss — shared by test_tail_ref_cpu.py, test_gpu_tail.py and
test_gpu_forward.py.  numpy / torch float64 only; nothing here touches a GPU.

* upsample_emulated  ATen's CPU bilinear align_corners=True arithmetic in fp32,
                     operation by operation (the kernel must give these bits).
* head_bwd_ref       sigmoid backward in fp64 from the fp32 heat, then the exact
                     adjoint of the fp64 upsample (autograd).
* head_fc_bwd_ref    the 1x1 scoring conv's three gradients as fp64 einsums.
* loss_ref           nn.BCELoss / nn.MSELoss on p.double(), gradient by autograd,
                     cast to fp32 (the .double() cast's backward).
* saturated_block    the BCE inputs on which both ATen clamps act.
"""
import numpy as np
import torch
import torch.nn.functional as F

# n, k, h, w -> H, W: what each reaches in upsample_sigmoid_kernel / head_bwd
UPSAMPLE_SHAPES = [
    (1, 2, 10, 13, 75, 101),   # W % 4 = 1 (ROW4 = false), two blocks, 7575 % 4 = 3 (partial last thread)
    (2, 1, 3, 5, 17, 23),      # small, odd W
    (1, 1, 9, 7, 9, 7),        # in == out on both axes
    (1, 2, 12, 16, 12, 128),   # in == out on rows only
    (1, 2, 1, 5, 9, 40),       # h = 1
    (1, 2, 4, 1, 32, 6),       # w = 1
    (1, 1, 1, 1, 5, 7),        # h = w = 1
    (1, 2, 5, 6, 1, 24),       # H = 1 (forward only: the backward needs H >= h)
]


def rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def upsample_emulated(low, H, W):
    """The exact fp32 arithmetic of ATen's CPU bilinear align_corners=True kernel
    as measured on the fixture-generating host (torch 2.10, contracted form
    t = fma(x0, l0, x1*l1)); host-ISA independent, so it pins the GPU bitwise.
    The scale is ATen's area_pixel_compute_scale: (in-1)/(out-1) in fp32, and 0
    for a single output (so out == 1 reads node 0, and in == 1 gives scale 0)."""
    f = np.float32
    x = low.numpy().astype(f)
    h, w = x.shape[2:]

    def idx(inn, out):
        scale = f(inn - 1) / f(out - 1) if out > 1 else f(0)
        src = (scale * np.arange(out, dtype=f)).astype(f)
        i0 = np.minimum(np.floor(src).astype(np.int64), inn - 1)
        l1 = np.clip((src - i0.astype(f)).astype(f), f(0), f(1))
        return i0, i0 + (i0 < inn - 1), (f(1) - l1).astype(f), l1

    def fma(a, b, c):
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f)

    h0, h1, lh0, lh1 = idx(h, H)
    w0, w1, lw0, lw1 = idx(w, W)

    def row(hi):
        return fma(x[:, :, hi][..., w0], lw0, (x[:, :, hi][..., w1] * lw1).astype(f))
    return torch.from_numpy(fma(row(h0), lh0[:, None], (row(h1) * lh1[:, None]).astype(f)))


def head_bwd_ref(g, heat, h, w):
    """dlow [N,K,h,w] float64: dz = g * (1 - p) * p in fp64 from the fp32 heat p
    (heat None: g already is dz), then the adjoint of
    F.interpolate(., (H, W), bilinear, align_corners=True) taken by fp64 autograd."""
    dz = g.double()
    if heat is not None:
        p = heat.double()
        dz = dz * (1.0 - p) * p
    n, k, H, W = g.shape
    low = torch.zeros(n, k, h, w, dtype=torch.float64, requires_grad=True)
    F.interpolate(low, size=(H, W), mode="bilinear", align_corners=True).backward(dz)
    return low.grad


def head_fc_bwd_ref(dlow, feat, w_kc):
    """dlow [N,K,h,w], feat NHWC [N,h,w,C], w [K,C] -> (dfeat NHWC, dw [K,C], db [K]), float64."""
    d, f, wt = dlow.double(), feat.double(), w_kc.double()
    return (torch.einsum("nkhw,kc->nhwc", d, wt), torch.einsum("nkhw,nhwc->kc", d, f),
            torch.einsum("nkhw->k", d))


def loss_ref(p_f32, target_f64, kind):
    """(loss float64 0-dim, dL/dp float32): nn.BCELoss / nn.MSELoss (mean) on
    p.double() against the fp64 target; the gradient is autograd's, cast to fp32
    by the .double() cast's own backward."""
    assert p_f32.dtype == torch.float32 and target_f64.dtype == torch.float64
    p = p_f32.detach().clone().requires_grad_(True)
    fn = {"bce": torch.nn.BCELoss, "mse": torch.nn.MSELoss}[kind]()
    loss = fn(p.double(), target_f64)
    loss.backward()
    return loss.detach(), p.grad


def saturated_block(seed=0):
    """(p fp32, target fp64), both [1,1,200,200]: a quarter each of p is exactly 0,
    exactly 1, rand * 1e-13 and 1 - rand * 2e-7 (shuffled over the plane) — where
    BCE's log clamp (-100) and its gradient's denominator clamp act, as on the
    saturated pixels of a trained net.  Target uniform in [0,1], one row exactly
    0 and one row exactly 1."""
    g = torch.Generator().manual_seed(seed)
    n = 200 * 200
    q = n // 4
    r = torch.rand(n, generator=g)
    p = torch.empty(n)
    p[:q] = 0.0
    p[q:2 * q] = 1.0
    p[2 * q:3 * q] = r[2 * q:3 * q] * 1e-13
    p[3 * q:] = 1.0 - r[3 * q:] * 2e-7
    p = p[torch.randperm(n, generator=g)].reshape(1, 1, 200, 200).contiguous()
    y = torch.rand(1, 1, 200, 200, generator=g, dtype=torch.float64)
    y[0, 0, 17] = 0.0
    y[0, 0, 101] = 1.0
    return p, y
