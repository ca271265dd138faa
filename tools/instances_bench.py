#!/usr/bin/env python3
"""HIP-event time of the multi-instance loss launch (hkp_heat_loss_multi: BCE, with
dheat, absent="zero") at M = 1, 4 and 16 instances per plane, next to the existing
single-instance launch (hkp_heat_loss from uv) on the same heatmaps — all in the
same process.  Default shape: the C3 shard's tail, B=8, K=4, 480x640.

Warm-up, then `--windows` windows of `--window-ms` of back-to-back launches each
(events around the window, launch count calibrated from the warm-up), all of them
alternating so that all see the same machine state; the median window gives the
time per call.  Every slot is present (the worst case for the inner loop); the M = 1
labels are the uv labels.  Before timing, the M = 1 gradient is compared bit for bit
with the existing launch's.  The yardstick for M = 1 is the existing launch, the
margin that launch's own window-to-window spread.  Prints one line and a JSON
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

MS = (1, 4, 16)


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
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--window-ms", type=float, default=300.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("instances_bench: no GPU (there is no CPU path to time)")
    from hkp import _lib
    dev = torch.device("cuda", 0)
    B, K, H, W = args.batch, args.keypoints, args.height, args.width
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731
    g = torch.Generator().manual_seed(1)
    heat = torch.rand(B, K, H, W, generator=g).clamp_(1e-6, 1 - 1e-6).to(dev)
    pts = torch.empty(B, K, max(MS), 3)
    pts[..., 0] = torch.rand(B, K, max(MS), generator=g) * (W - 1)
    pts[..., 1] = torch.rand(B, K, max(MS), generator=g) * (H - 1)
    pts[..., 2] = 1.0
    labels = {m: pts[:, :, :m].contiguous().to(dev) for m in MS}
    uv = pts[:, :, 0, :2].contiguous().to(dev)
    loss = torch.empty((), device=dev, dtype=torch.float64)
    dheat = torch.empty_like(heat)
    dheat_old = torch.empty_like(heat)
    ws_old = torch.empty(_lib.lib().hkp_heat_loss_workspace() // 8, device=dev, dtype=torch.float64)
    ws = torch.empty(_lib.lib().hkp_heat_loss_multi_workspace(B, K, H, W) // 8, device=dev, dtype=torch.float64)

    def old():
        _lib.call("hkp_heat_loss", B, K, H, W, _lib.HKP_LOSS_BCE, P(heat), None, P(uv), args.sigma, P(loss),
                  P(dheat_old), P(ws_old), stream)

    def multi(m):
        return lambda: _lib.call("hkp_heat_loss_multi", B, K, m, H, W, _lib.HKP_LOSS_BCE, _lib.HKP_ABSENT_ZERO, P(heat),
                                 P(labels[m]), args.sigma, P(loss), P(dheat), P(ws), stream)

    old()
    multi(1)()
    torch.cuda.synchronize()
    if not torch.equal(dheat, dheat_old):
        sys.exit("instances_bench: the M = 1 gradient differs from hkp_heat_loss's")
    names = ["heat_loss_uv"] + ["multi_m%d" % m for m in MS]
    fns = [old] + [multi(m) for m in MS]
    for fn in fns:                                   # warm-up, and the calibration of the window length
        _window(fn, 20)
    iters = [max(20, int(args.window_ms / _window(fn, 50))) for fn in fns]
    times = [[] for _ in fns]
    for _ in range(args.windows):                    # alternating: all see the same machine state
        for t, fn, n in zip(times, fns, iters):
            t.append(_window(fn, n))
    med = [_median(t) for t in times]
    print("  ".join("%s %.2f us" % (k, 1e3 * m) for k, m in zip(names, med)), flush=True)
    print(json.dumps({"tool": "instances_bench", "device": torch.cuda.get_device_name(0), "batch": B, "keypoints": K,
                      "height": H, "width": W, "sigma": args.sigma, "windows": args.windows,
                      "window_ms": args.window_ms, "us": {k: 1e3 * m for k, m in zip(names, med)},
                      "over_heat_loss_uv": {k: m / med[0] for k, m in zip(names[1:], med[1:])},
                      "spread_us": {k: [1e3 * min(t), 1e3 * max(t)] for k, t in zip(names, times)},
                      "heat_loss_uv_spread_rel": (max(times[0]) - min(times[0])) / med[0],
                      "launches_per_window": iters}))


if __name__ == "__main__":
    main()
