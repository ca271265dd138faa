#!/usr/bin/env python3
"""HIP-event time of the multi-peak decode launch (hkp_heat_peaks) alone, at
(radius 1, max_peaks 4) and at (radius 8, max_peaks 16) — and at (1, 16) and (8, 1),
which separate the window test from the selection rounds — next to the existing
argmax-only decode (hkp_upsample_sigmoid with heat = NULL: upsample + sigmoid +
argmax, two launches) on the same low-res logits — all in the same process.
Default shape: the C2 decode, B=32, K=4, 60x80 -> 480x640.

Warm-up, then `--windows` windows of `--window-ms` of back-to-back launches each
(events around the window, launch count calibrated from the warm-up), all of them
alternating so that all see the same machine state; the median window gives the
time per call.  Two inputs: seeded N(0,1) logits (an untrained head: many local
maxima) and the logits of one Gaussian per plane (a trained head).  The peaks
are compared with the numpy restatement (tests/_peaks_ref.py) first.  Prints one
line per input and a JSON summary; not a gate."""
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


# (radius, max_peaks): the two the comparison is about, and the two crossed ones, which
# tell the window test's cost (radius) from the selection rounds' (max_peaks)
CONFIGS = [(1, 4), (8, 16), (1, 16), (8, 1)]


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


def gaussian_logits(B, K, h, w, H, W, sigma, seed):
    rng = np.random.default_rng(seed)
    ys = np.arange(h) * (H - 1) / max(h - 1, 1)
    xs = np.arange(w) * (W - 1) / max(w - 1, 1)
    cy, cx = rng.uniform(0, H - 1, (B, K, 1, 1)), rng.uniform(0, W - 1, (B, K, 1, 1))
    p = np.clip(np.exp(-((ys[:, None] - cy) ** 2 + (xs[None, :] - cx) ** 2) / (2.0 * sigma * sigma)), 1e-30, 1 - 2.0 ** -24)
    return (np.log(p) - np.log1p(-p)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--keypoints", type=int, default=4)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--window-ms", type=float, default=300.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("peaks_bench: no GPU (there is no CPU path to time)")
    import _peaks_ref as ref
    from hkp import _lib, ops
    dev = torch.device("cuda", 0)
    B, K, H, W = args.batch, args.keypoints, args.height, args.width
    h, w = H // 8, W // 8
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731
    inputs = {"normal": np.random.default_rng(1).normal(0, 1, (B, K, h, w)).astype(np.float32),
              "gaussian": gaussian_logits(B, K, h, w, H, W, 8.0, 2)}
    ws = torch.empty(_lib.lib().hkp_upsample_argmax_ws_bytes(B, K, H, W) // 8, device=dev, dtype=torch.int64)
    yx = torch.empty((B, K, 2), device=dev, dtype=torch.int32)
    pk = {p: torch.empty((B, K, p, 3), device=dev) for p in sorted({p for _, p in CONFIGS})}
    ct = torch.empty((B, K), device=dev, dtype=torch.int32)
    results = {}
    for name, low_np in inputs.items():
        low = torch.from_numpy(low_np).to(dev)

        def argmax():
            _lib.call("hkp_upsample_sigmoid", B, K, h, w, H, W, 1, P(low), None, P(ws), P(yx), stream)

        def peaks(r, p, out):
            return lambda: _lib.call("hkp_heat_peaks", B, K, h, w, H, W, r, p, 0.0, P(low), P(out), P(ct), stream)

        scores = ops.upsample_sigmoid(low, h, w, heat=True, argmax=False)[0].cpu().numpy()
        mean_count = {}
        for r, p in CONFIGS:
            peaks(r, p, pk[p])()
            torch.cuda.synchronize()
            want, want_c = ref.heat_peaks(low_np[:2], H, W, max_peaks=p, radius=r, scores=scores[:2])
            got = pk[p][:2].cpu().numpy()
            if not np.array_equal(ct[:2].cpu().numpy(), want_c) or np.abs(got - want).max() > np.spacing(np.float32(max(H, W))):
                sys.exit("peaks_bench: %s differs from the restatement (radius %d, max_peaks %d)" % (name, r, p))
            mean_count["r%d_p%d" % (r, p)] = float(ct.float().mean().item())

        names = ["argmax_decode"] + ["peaks_r%d_p%d" % c for c in CONFIGS]
        fns = [argmax] + [peaks(r, p, pk[p]) for r, p in CONFIGS]
        for fn in fns:                                   # warm-up, and the calibration of the window length
            _window(fn, 20)
        iters = [max(20, int(args.window_ms / _window(fn, 50))) for fn in fns]
        times = [[] for _ in fns]
        for _ in range(args.windows):                    # alternating: all see the same machine state
            for t, fn, n in zip(times, fns, iters):
                t.append(_window(fn, n))
        med = [_median(t) for t in times]
        results[name] = {"us": {k: 1e3 * m for k, m in zip(names, med)},
                         "over_argmax": {k: m / med[0] for k, m in zip(names[1:], med[1:])},
                         "spread_us": {k: [1e3 * min(t), 1e3 * max(t)] for k, t in zip(names, times)},
                         "launches_per_window": iters, "mean_peaks_per_plane": mean_count}
        print("%-9s " % name + "  ".join("%s %.2f us" % (k, 1e3 * m) for k, m in zip(names, med)), flush=True)
    print(json.dumps({"tool": "peaks_bench", "device": torch.cuda.get_device_name(0), "batch": B, "keypoints": K,
                      "height": H, "width": W, "lowres": [h, w], "windows": args.windows, "window_ms": args.window_ms,
                      "inputs": results}))


if __name__ == "__main__":
    main()
