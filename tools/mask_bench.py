#!/usr/bin/env python3
"""HIP-event time of the masked loss entry (hkp_heat_loss_masked, BCE, with dheat,
absent="zero", the elements divisor) next to hkp_heat_loss_planes on the same heatmaps and
labels, and of the two mask kernels next to a clone() of the mask — all in the same
process.  Default shape: the C3 shard's tail, B=8, K=4, 480x640, one present instance per
plane.  The forms:

  planes      hkp_heat_loss_planes, weights NULL, topk 0: the yardstick (existing code)
  zero_mask   hkp_heat_loss_masked with an all-zero mask: one more byte per 8 B element and
              the count pass over N*H*W bytes
  mask30      ... with about 30 % of the pixels masked per class bit
  mask30_top2 ... and topk = 2 of the K classes: two passes, the second on half the planes
  regions     hkp_mask_regions_u8, R = 8 regions per image
  warp        hkp_warp_mask_u8, a rotation by 10 degrees about the centre, constant border
  clone       mask.clone(): the copy of N*H*W bytes the two above are read against

Warm-up, then `--windows` windows of `--window-ms` of back-to-back launches each (events
around the window, launch count calibrated from the warm-up), the forms alternating so
that all see the same machine state; the median window gives the time per call.  Before
timing, the all-zero form is compared bit for bit with hkp_heat_loss_planes, and the
top-k form's plane_used is checked to hold 2 planes per image.  Prints one line and a JSON
summary; a record, not a gate."""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "hulk-keypoints_amd"))

import torch  # noqa: E402

NAMES = ("planes", "zero_mask", "mask30", "mask30_top2", "regions", "warp", "clone")


def _window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--keypoints", type=int, default=4)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--sigma", type=float, default=8.0)
    ap.add_argument("--topk", type=int, default=2)
    ap.add_argument("--regions", type=int, default=8)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--window-ms", type=float, default=300.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mask_bench: no GPU (there is no CPU path to time)")
    from hkp import _lib, geometry, masks, ops
    dev = torch.device("cuda", 0)
    B, K, H, W = args.batch, args.keypoints, args.height, args.width
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731
    g = torch.Generator().manual_seed(1)
    heat = torch.rand(B, K, H, W, generator=g).clamp_(1e-6, 1 - 1e-6).to(dev)
    pts = torch.empty(B, K, 1, 3)
    pts[..., 0] = torch.rand(B, K, 1, generator=g) * (W - 1)
    pts[..., 1] = torch.rand(B, K, 1, generator=g) * (H - 1)
    pts[..., 2] = 1.0
    pts = pts.to(dev)
    zero = torch.zeros(B, H, W, dtype=torch.uint8, device=dev)
    m30 = torch.zeros(B, H, W, dtype=torch.int64)
    for c in range(8):
        m30 |= (torch.rand(B, H, W, generator=g) < 0.3).long() << c
    m30 = m30.to(torch.uint8).to(dev)
    loss = torch.empty((), device=dev, dtype=torch.float64)
    loss_pl = torch.empty((), device=dev, dtype=torch.float64)
    dheat = torch.empty_like(heat)
    dheat_pl = torch.empty_like(heat)
    plane_loss = torch.empty(B, K, device=dev, dtype=torch.float64)
    plane_used = torch.empty(B, K, device=dev, dtype=torch.int32)
    plane_pixels = torch.empty(B, K, device=dev, dtype=torch.int32)
    ws_pl = torch.empty(_lib.lib().hkp_heat_loss_planes_workspace(B, K, H, W) // 8, device=dev, dtype=torch.float64)
    ws = torch.empty(_lib.lib().hkp_heat_loss_masked_workspace(B, K, H, W) // 8, device=dev, dtype=torch.float64)

    def planes():
        _lib.call("hkp_heat_loss_planes", B, K, 1, H, W, _lib.HKP_LOSS_BCE, _lib.HKP_ABSENT_ZERO,
                  _lib.HKP_NORM_ELEMENTS, 2.0, 0, P(heat), P(pts), None, args.sigma, P(loss_pl), P(dheat_pl),
                  P(plane_loss), P(plane_used), P(ws_pl), stream)

    def masked(mask, topk):
        return lambda: _lib.call("hkp_heat_loss_masked", B, K, 1, H, W, _lib.HKP_LOSS_BCE, _lib.HKP_ABSENT_ZERO,
                                 _lib.HKP_NORM_ELEMENTS, 2.0, topk, P(heat), P(pts), None, P(mask), args.sigma,
                                 P(loss), P(dheat), P(plane_loss), P(plane_used), P(plane_pixels), P(ws), stream)

    rg = [[masks.disc(float(torch.rand(1, generator=g)) * W, float(torch.rand(1, generator=g)) * H, 20 + 5 * j, j % K)
           if j % 2 else masks.box(10 * j, 8 * j, 10 * j + 100, 8 * j + 60, (j % K,)) for j in range(args.regions)]
          for _ in range(B)]
    regs = masks.pack(rg, R=args.regions, device=dev)
    raster_out = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
    plan = geometry.WarpPlan([geometry.affine_matrix(H, W, rotate_deg=10.0)] * B, (H, W), border="constant")
    xf = plan.device_array(dev)
    warp_out = torch.empty(B, H, W, dtype=torch.uint8, device=dev)

    def regions():
        _lib.call("hkp_mask_regions_u8", B, args.regions, H, W, P(regs), P(raster_out), stream)

    def warp():
        _lib.call("hkp_warp_mask_u8", B, H, W, P(m30), H, W, P(warp_out), plan.xforms, P(xf), plan.border, 0, None,
                  stream)

    fns = [planes, masked(zero, 0), masked(m30, 0), masked(m30, args.topk), regions, warp, lambda: m30.clone()]
    planes()                                         # the two checks before any timing
    fns[1]()
    torch.cuda.synchronize()
    if not torch.equal(dheat, dheat_pl) or loss.item() != loss_pl.item():
        sys.exit("mask_bench: hkp_heat_loss_masked with an all-zero mask differs from hkp_heat_loss_planes")
    if plane_pixels.tolist() != [[H * W] * K] * B:
        sys.exit("mask_bench: plane_pixels of an all-zero mask is not H*W")
    fns[3]()
    torch.cuda.synchronize()
    if plane_used.sum(1).tolist() != [args.topk] * B:
        sys.exit("mask_bench: topk did not count %d planes per image" % args.topk)
    kept = float(plane_pixels.sum().item()) / (B * K * H * W)
    regions()
    set_px = float((ops.mask_regions_u8(regs, H, W) != 0).float().mean().item())
    for fn in fns:                                   # warm-up, and the calibration of the window length
        _window(fn, 20)
    iters = [max(20, int(args.window_ms / _window(fn, 50))) for fn in fns]
    times = [[] for _ in fns]
    for _ in range(args.windows):                    # alternating: all see the same machine state
        for t, fn, n in zip(times, fns, iters):
            t.append(_window(fn, n))
    med = [_median(t) for t in times]
    print("  ".join("%s %.2f us" % (k, 1e3 * v) for k, v in zip(NAMES, med)), flush=True)
    result = {"us": {k: 1e3 * v for k, v in zip(NAMES, med)},
              "over_planes": {k: v / med[0] for k, v in zip(NAMES[1:4], med[1:4])},
              "over_clone": {k: v / med[6] for k, v in zip(NAMES[4:6], med[4:6])},
              "spread_us": {k: [1e3 * min(t), 1e3 * max(t)] for k, t in zip(NAMES, times)},
              "spread_rel": {k: (max(t) - min(t)) / m for k, t, m in zip(NAMES, times, med)},
              "kept_fraction_mask30": kept, "set_fraction_regions": set_px, "launches_per_window": iters}
    print(json.dumps({"tool": "mask_bench", "device": torch.cuda.get_device_name(0), "batch": B, "keypoints": K,
                      "height": H, "width": W, "sigma": args.sigma, "topk": args.topk, "regions": args.regions,
                      "windows": args.windows, "window_ms": args.window_ms, "results": result}))


if __name__ == "__main__":
    main()
