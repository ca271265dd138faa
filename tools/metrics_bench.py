#!/usr/bin/env python3
"""HIP-event time of the evaluation launch (hkp_peaks_match) alone, at
(B, K, P, M, T) = (32, 4, 4, 4, 4) and (32, 4, 16, 16, 8), with and without the
per-batch outputs, next to the multi-peak decode that feeds it (hkp_heat_peaks on
60x80 logits of the same batch, max_peaks 4 and 16) — all in the same process.

Warm-up, then `--windows` windows of `--window-ms` of back-to-back launches each
(events around the window, launch count calibrated from the warm-up), all of them
alternating so that all see the same machine state; the median window gives the
time per call.  The matched inputs are the seeded planes of the tests
(tests/_metrics_ref.py: instances, peaks near them, strays, absent planes); the
kernel's integers are compared with the numpy restatement on the first two batch
rows first.  Prints one line and a JSON summary; not a gate."""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "hulk-keypoints_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

# (P, M, thresholds)
CONFIGS = [(4, 4, (2.0, 4.0, 8.0, 16.0)), (16, 16, (1.0, 2.0, 3.0, 4.0, 6.0, 8.0, 12.0, 16.0))]
BINS = 1024


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
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--keypoints", type=int, default=4)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--window-ms", type=float, default=200.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("metrics_bench: no GPU (there is no CPU path to time)")
    import _metrics_ref as ref
    from hkp import _lib
    dev = torch.device("cuda", 0)
    B, K, H, W = args.batch, args.keypoints, args.height, args.width
    h, w = H // 8, W // 8
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731
    low = torch.from_numpy(np.random.default_rng(1).normal(0, 1, (B, K, h, w)).astype(np.float32)).to(dev)
    names, fns, keep = [], [], []
    for p, m, th in CONFIGS:
        t = len(th)
        pk_np, ct_np, lab_np = ref.random_batch(7 + p, B, K, p, m, size=float(min(H, W)))
        pk, ct, lab = (torch.from_numpy(a).to(dev) for a in (pk_np, ct_np, lab_np))
        hist = torch.zeros((K, t, 2, BINS), device=dev, dtype=torch.int64)
        totals = torch.zeros((K, 8), device=dev, dtype=torch.int64)
        pm = torch.empty((B, K, t, p), device=dev, dtype=torch.int32)
        gm = torch.empty((B, K, m), device=dev, dtype=torch.int32)
        gd = torch.empty((B, K, m), device=dev, dtype=torch.float32)
        tha = (ctypes.c_float * t)(*th)
        dpk = torch.empty((B, K, p, 3), device=dev)
        dct = torch.empty((B, K), device=dev, dtype=torch.int32)
        keep.append((pk, ct, lab, hist, totals, pm, gm, gd, tha, dpk, dct))

        def match(outputs, n=B, p=p, m=m, t=t, tha=tha, pk=pk, ct=ct, lab=lab, hist=hist, totals=totals, pm=pm, gm=gm,
                  gd=gd):
            o = (P(pm), P(gm), P(gd)) if outputs else (None, None, None)
            return lambda: _lib.call("hkp_peaks_match", n, K, p, m, t, BINS, tha, P(pk), P(ct), P(lab), P(hist),
                                     P(totals), o[0], o[1], o[2], stream)

        def decode(p=p, dpk=dpk, dct=dct):
            return lambda: _lib.call("hkp_heat_peaks", B, K, h, w, H, W, 1, p, 0.0, P(low), P(dpk), P(dct), stream)

        # the kernel against the restatement on the first two batch rows
        match(True, n=2)()
        torch.cuda.synchronize()
        want = ref.peaks_match(pk_np[:2], ct_np[:2], lab_np[:2], th, bins=BINS)
        same = (np.array_equal(hist.cpu().numpy(), want[0]) and np.array_equal(totals.cpu().numpy()[:, :5], want[1][:, :5])
                and np.array_equal(pm[:2].cpu().numpy(), want[2]) and np.array_equal(gm[:2].cpu().numpy(), want[3]))
        if not same:
            sys.exit("metrics_bench: the kernel differs from the restatement (P %d, M %d, T %d)" % (p, m, t))
        hist.zero_()
        totals.zero_()
        tag = "p%d_m%d_t%d" % (p, m, t)
        names += ["match_" + tag, "match_" + tag + "_outputs", "heat_peaks_r1_p%d" % p]
        fns += [match(False), match(True), decode()]
    for fn in fns:                                   # warm-up, and the calibration of the window length
        _window(fn, 20)
    iters = [max(20, int(args.window_ms / _window(fn, 50))) for fn in fns]
    times = [[] for _ in fns]
    for _ in range(args.windows):                    # alternating: all see the same machine state
        for t, fn, n in zip(times, fns, iters):
            t.append(_window(fn, n))
    med = [_median(t) for t in times]
    print("  ".join("%s %.2f us" % (k, 1e3 * v) for k, v in zip(names, med)), flush=True)
    print(json.dumps({"tool": "metrics_bench", "device": torch.cuda.get_device_name(0), "batch": B, "keypoints": K,
                      "height": H, "width": W, "lowres": [h, w], "bins": BINS, "windows": args.windows,
                      "window_ms": args.window_ms, "us": {k: 1e3 * v for k, v in zip(names, med)},
                      "spread_us": {k: [1e3 * min(t), 1e3 * max(t)] for k, t in zip(names, times)},
                      "launches_per_window": iters}))


if __name__ == "__main__":
    main()
