#!/usr/bin/env python3
"""HIP-event time of the quality focal loss launch (hkp_heat_loss_multi_ex, HKP_LOSS_QFL,
with dheat, absent="zero", the elements divisor) at beta = 2 (its own instantiation: no
pow) and beta = 1.5 (the general path: one fp64 pow per pixel), next to the BCE launch
(hkp_heat_loss_multi) on the same heatmaps and labels — all in the same process, at
M = 1 and M = 4 instances per plane.  Default shape: the C3 shard's tail, B=8, K=4,
480x640.

Warm-up, then `--windows` windows of `--window-ms` of back-to-back launches each (events
around the window, launch count calibrated from the warm-up), all of them alternating so
that all see the same machine state; the median window gives the time per call.  Every
slot is present.  Before timing, BCE through hkp_heat_loss_multi_ex is compared bit for
bit with hkp_heat_loss_multi, and the QFL loss at heat == target is checked to be 0.
The yardstick is the BCE launch of the same process and the same M.  Prints one line
per M and a JSON summary; not a gate."""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "hulk-keypoints_amd"))

import torch  # noqa: E402

MS = (1, 4)
KINDS = (("bce", None), ("qfl_beta2", 2.0), ("qfl_beta1.5", 1.5))


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
        sys.exit("focal_bench: no GPU (there is no CPU path to time)")
    from hkp import _lib, ops
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
    loss = torch.empty((), device=dev, dtype=torch.float64)
    dheat = torch.empty_like(heat)
    dheat_ex = torch.empty_like(heat)
    ws = torch.empty(_lib.lib().hkp_heat_loss_multi_workspace(B, K, H, W) // 8, device=dev, dtype=torch.float64)

    def bce(m):
        return lambda: _lib.call("hkp_heat_loss_multi", B, K, m, H, W, _lib.HKP_LOSS_BCE, _lib.HKP_ABSENT_ZERO, P(heat),
                                 P(labels[m]), args.sigma, P(loss), P(dheat), P(ws), stream)

    def ex(m, kind, beta, out):
        return lambda: _lib.call("hkp_heat_loss_multi_ex", B, K, m, H, W, kind, _lib.HKP_ABSENT_ZERO,
                                 _lib.HKP_NORM_ELEMENTS, beta, P(heat), P(labels[m]), args.sigma, P(loss), P(out),
                                 P(ws), stream)

    for m in MS:                                     # the two checks before any timing
        bce(m)()
        ex(m, _lib.HKP_LOSS_BCE, 2.0, dheat_ex)()
        torch.cuda.synchronize()
        if not torch.equal(dheat, dheat_ex):
            sys.exit("focal_bench: BCE through hkp_heat_loss_multi_ex differs from hkp_heat_loss_multi's")
        at = ops.gauss_target_multi(labels[m], H, W, args.sigma).float()
        for beta in (2.0, 1.5):
            l0, g0 = ops.heat_loss_multi(at, labels[m], args.sigma, "qfl", beta=beta)
            if l0.item() != 0.0 or g0.abs().max().item() != 0.0:
                sys.exit("focal_bench: the loss at heat == target is not 0 (beta %g)" % beta)
    result = {}
    for m in MS:
        names = [k for k, _ in KINDS]
        fns = [bce(m)] + [ex(m, _lib.HKP_LOSS_QFL, beta, dheat) for _, beta in KINDS[1:]]
        for fn in fns:                               # warm-up, and the calibration of the window length
            _window(fn, 20)
        iters = [max(20, int(args.window_ms / _window(fn, 50))) for fn in fns]
        times = [[] for _ in fns]
        for _ in range(args.windows):                # alternating: all see the same machine state
            for t, fn, n in zip(times, fns, iters):
                t.append(_window(fn, n))
        med = [_median(t) for t in times]
        print("M=%d  " % m + "  ".join("%s %.2f us (x%.3f)" % (k, 1e3 * v, v / med[0]) for k, v in zip(names, med)),
              flush=True)
        result["m%d" % m] = {"us": {k: 1e3 * v for k, v in zip(names, med)},
                             "over_bce": {k: v / med[0] for k, v in zip(names[1:], med[1:])},
                             "spread_us": {k: [1e3 * min(t), 1e3 * max(t)] for k, t in zip(names, times)},
                             "bce_spread_rel": (max(times[0]) - min(times[0])) / med[0],
                             "launches_per_window": iters}
    print(json.dumps({"tool": "focal_bench", "device": torch.cuda.get_device_name(0), "batch": B, "keypoints": K,
                      "height": H, "width": W, "sigma": args.sigma, "windows": args.windows,
                      "window_ms": args.window_ms, "results": result}))


if __name__ == "__main__":
    main()
