#!/usr/bin/env python3
"""HIP-event time of the domain-randomisation launch (hkp_augment_u8) alone at
B=32, 640x480, next to a clone() of the same uint8 tensor in the same process: a
device copy moves the same 6 B/pixel (3 read + 3 written), so it is the yardstick
for a kernel that is bound by memory traffic.

Per case: warm-up, then `--windows` windows of `--window-ms` of back-to-back
launches each (events around the window, launch count calibrated from the
warm-up), clone and augment windows alternating; the median window gives the
time per launch.  Cases: the sampled reference programs (all eight operators),
the same without BLUR (no halo, no fp32 pass), and empty programs (the kernel's
load / store skeleton).  Prints one line per case and a JSON summary; not a gate."""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "hulk-keypoints_amd"))

import torch  # noqa: E402


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
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=500.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("augment_bench: no GPU (there is no CPU path to time)")
    from hkp import _lib, augment
    from oracle import recipe
    dev = torch.device("cuda", 0)
    B, H, W = args.batch, args.height, args.width
    x = torch.from_numpy(recipe.seeded_images_u8(B, H, W, 5)).to(dev)
    out = torch.empty_like(x)
    table = augment.TABLE.on(dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731

    cases = {
        "reference programs": augment.DomainRandomization(seed=0).plan(range(B), 0),
        "without BLUR": augment.DomainRandomization(seed=0, ops={"blur": None}).plan(range(B), 0),
        "empty programs": augment.Plan.from_stages([[] for _ in range(B)]),
    }
    # one operator of each stage kind alone (random_order is moot): what each phase costs
    for op in ("gamma", "hue_sat", "blur", "noise"):
        cases[op + " alone"] = augment.DomainRandomization(seed=0, ops=[op]).plan(range(B), 0)

    def clone():
        x.clone()

    results = {}
    for name, plan in cases.items():
        progs, luts = plan.device_arrays(dev)

        def launch():
            _lib.call("hkp_augment_u8", B, H, W, P(x), P(out), plan.programs, P(progs), P(luts), P(table), stream)

        torch.cuda.synchronize()
        for fn in (clone, launch):                       # warm-up, and the calibration of the window length
            _window(fn, 20)
        n_clone = max(20, int(args.window_ms / _window(clone, 50)))
        n_aug = max(20, int(args.window_ms / _window(launch, 50)))
        t_clone, t_aug = [], []
        for _ in range(args.windows):                    # alternating: both see the same machine state
            t_clone.append(_window(clone, n_clone))
            t_aug.append(_window(launch, n_aug))
        c, a = _median(t_clone), _median(t_aug)
        gbs = 6.0 * B * H * W / 1e6                      # MB moved at 6 B/pixel; / ms = GB/s
        results[name] = {"augment_ms": a, "clone_ms": c, "ratio": a / c, "augment_GBps": gbs / a,
                         "clone_GBps": gbs / c, "augment_spread": [min(t_aug), max(t_aug)],
                         "clone_spread": [min(t_clone), max(t_clone)], "launches_per_window": [n_aug, n_clone]}
        print("%-20s augment %.4f ms (%.0f GB/s)  clone %.4f ms (%.0f GB/s)  ratio %.2f" % (
            name, a, gbs / a, c, gbs / c, a / c), flush=True)
    print(json.dumps({"tool": "augment_bench", "device": torch.cuda.get_device_name(0), "batch": B, "height": H,
                      "width": W, "windows": args.windows, "window_ms": args.window_ms, "cases": results}))


if __name__ == "__main__":
    main()
