#!/usr/bin/env python3
"""HIP-event time of the plane-weighted loss entry (hkp_heat_loss_planes, BCE, with dheat,
absent="zero", the elements divisor) next to the BCE launch of hkp_heat_loss_multi_ex on the
same heatmaps and labels — all in the same process.  Default shape: the C3 shard's tail,
B=8, K=4, 480x640, one present instance per plane.  Four forms:

  multi_ex   hkp_heat_loss_multi_ex: the yardstick (existing code)
  planes     hkp_heat_loss_planes, weights NULL, topk 0: one pass plus two one-block kernels
  weights    ... with a weight per plane in [0.25, 1.75)
  topk2      ... with topk = 2 of the K classes: two passes, the second on half the planes

Warm-up, then `--windows` windows of `--window-ms` of back-to-back launches each (events
around the window, launch count calibrated from the warm-up), the forms alternating so
that all see the same machine state; the median window gives the time per call.  Before
timing, the weights-NULL form is compared bit for bit with hkp_heat_loss_multi_ex, and the
topk form's plane_used is checked to hold 2 planes per image.  Prints one line and a JSON
summary; not a gate."""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "hulk-keypoints_amd"))

import torch  # noqa: E402

NAMES = ("multi_ex", "planes", "weights", "topk2")


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
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--window-ms", type=float, default=300.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("planes_bench: no GPU (there is no CPU path to time)")
    from hkp import _lib
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
    weights = (torch.rand(B, K, generator=g) * 1.5 + 0.25).to(dev)
    loss = torch.empty((), device=dev, dtype=torch.float64)
    dheat = torch.empty_like(heat)
    dheat_ex = torch.empty_like(heat)
    plane_loss = torch.empty(B, K, device=dev, dtype=torch.float64)
    plane_used = torch.empty(B, K, device=dev, dtype=torch.int32)
    ws_ex = torch.empty(_lib.lib().hkp_heat_loss_multi_workspace(B, K, H, W) // 8, device=dev, dtype=torch.float64)
    ws = torch.empty(_lib.lib().hkp_heat_loss_planes_workspace(B, K, H, W) // 8, device=dev, dtype=torch.float64)

    def ex():
        _lib.call("hkp_heat_loss_multi_ex", B, K, 1, H, W, _lib.HKP_LOSS_BCE, _lib.HKP_ABSENT_ZERO,
                  _lib.HKP_NORM_ELEMENTS, 2.0, P(heat), P(pts), args.sigma, P(loss), P(dheat_ex), P(ws_ex), stream)

    def planes(w, topk):
        return lambda: _lib.call("hkp_heat_loss_planes", B, K, 1, H, W, _lib.HKP_LOSS_BCE, _lib.HKP_ABSENT_ZERO,
                                 _lib.HKP_NORM_ELEMENTS, 2.0, topk, P(heat), P(pts), None if w is None else P(w),
                                 args.sigma, P(loss), P(dheat), P(plane_loss), P(plane_used), P(ws), stream)

    fns = [ex, planes(None, 0), planes(weights, 0), planes(weights, args.topk)]
    ex()                                             # the two checks before any timing
    l_ex = loss.item()
    fns[1]()
    torch.cuda.synchronize()
    if not torch.equal(dheat, dheat_ex):
        sys.exit("planes_bench: hkp_heat_loss_planes without weights differs from hkp_heat_loss_multi_ex")
    if abs(loss.item() - l_ex) > 1e-12 * abs(l_ex):
        sys.exit("planes_bench: the loss differs from hkp_heat_loss_multi_ex's")
    fns[3]()
    torch.cuda.synchronize()
    if plane_used.sum(1).tolist() != [args.topk] * B:
        sys.exit("planes_bench: topk did not count %d planes per image" % args.topk)
    for fn in fns:                                   # warm-up, and the calibration of the window length
        _window(fn, 20)
    iters = [max(20, int(args.window_ms / _window(fn, 50))) for fn in fns]
    times = [[] for _ in fns]
    for _ in range(args.windows):                    # alternating: all see the same machine state
        for t, fn, n in zip(times, fns, iters):
            t.append(_window(fn, n))
    med = [_median(t) for t in times]
    print("  ".join("%s %.2f us (x%.3f)" % (k, 1e3 * v, v / med[0]) for k, v in zip(NAMES, med)), flush=True)
    result = {"us": {k: 1e3 * v for k, v in zip(NAMES, med)},
              "over_multi_ex": {k: v / med[0] for k, v in zip(NAMES[1:], med[1:])},
              "spread_us": {k: [1e3 * min(t), 1e3 * max(t)] for k, t in zip(NAMES, times)},
              "spread_rel": {k: (max(t) - min(t)) / m for k, t, m in zip(NAMES, times, med)},
              "launches_per_window": iters}
    print(json.dumps({"tool": "planes_bench", "device": torch.cuda.get_device_name(0), "batch": B, "keypoints": K,
                      "height": H, "width": W, "sigma": args.sigma, "topk": args.topk, "windows": args.windows,
                      "window_ms": args.window_ms, "results": result}))


if __name__ == "__main__":
    main()
