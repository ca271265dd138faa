#!/usr/bin/env python3
"""HIP-event time of the affine-warp launch (hkp_warp_affine_u8) alone at B=32,
640x480, next to a clone() of the same uint8 tensor and next to the
domain-randomisation launch (hkp_augment_u8, the sampled reference programs) it
sits beside in the data path, all in the same process.  A device copy moves 6
B/pixel (3 read + 3 written): the yardstick for a kernel bound by memory traffic.
The warp requests 12 B per output pixel from the memory pipeline in bilinear mode
(four 3-byte taps, as byte loads) and 3 B in nearest mode; neighbouring pixels
share taps, so what leaves the caches stays near the image's 3 B/pixel.

Per case: warm-up, then `--windows` windows of `--window-ms` of back-to-back
launches each (events around the window, launch count calibrated from the
warm-up), with clone, augment and warp windows alternating; the median window
gives the time per launch.  Cases: a 15 degree rotation at scale 1.05 and a pure
hflip, bilinear and nearest, constant border.  Prints one line per case and a
JSON summary; not a gate."""
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
        sys.exit("warp_bench: no GPU (there is no CPU path to time)")
    from hkp import _lib, augment, geometry
    from oracle import recipe
    dev = torch.device("cuda", 0)
    B, H, W = args.batch, args.height, args.width
    x = torch.from_numpy(recipe.seeded_images_u8(B, H, W, 5)).to(dev)
    out = torch.empty_like(x)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731

    aplan = augment.DomainRandomization(seed=0).plan(range(B), 0)
    progs, luts = aplan.device_arrays(dev)
    table = augment.TABLE.on(dev)

    def clone():
        x.clone()

    def aug():
        _lib.call("hkp_augment_u8", B, H, W, P(x), P(out), aplan.programs, P(progs), P(luts), P(table), stream)

    rot = geometry.affine_matrix(H, W, rotate_deg=15, scale=1.05)
    flip = geometry.affine_matrix(H, W, hflip=True)
    cases = {}
    for name, m in (("rotate 15 scale 1.05", rot), ("hflip", flip)):
        for interp in ("bilinear", "nearest"):
            cases["%s, %s" % (name, interp)] = geometry.WarpPlan([m] * B, (H, W), interp=interp)

    results = {}
    for name, plan in cases.items():
        xf = plan.device_array(dev)

        def launch():
            _lib.call("hkp_warp_affine_u8", B, H, W, P(x), H, W, P(out), plan.xforms, P(xf), plan.interp, plan.border,
                      stream)

        torch.cuda.synchronize()
        fns = (clone, aug, launch)
        for fn in fns:                                   # warm-up, and the calibration of the window length
            _window(fn, 20)
        iters = [max(20, int(args.window_ms / _window(fn, 50))) for fn in fns]
        times = ([], [], [])
        for _ in range(args.windows):                    # alternating: all three see the same machine state
            for t, fn, n in zip(times, fns, iters):
                t.append(_window(fn, n))
        c, a, w = (_median(t) for t in times)
        mb = 6.0 * B * H * W / 1e6                       # MB moved at 6 B/pixel; / ms = GB/s
        requested = (12 if plan.interp == _lib.HKP_WARP_BILINEAR else 3) * B * H * W
        results[name] = {"warp_ms": w, "augment_ms": a, "clone_ms": c, "warp_over_clone": w / c,
                         "warp_over_augment": w / a, "warp_GBps": mb / w, "clone_GBps": mb / c,
                         "warp_spread": [min(times[2]), max(times[2])], "augment_spread": [min(times[1]), max(times[1])],
                         "clone_spread": [min(times[0]), max(times[0])], "launches_per_window": iters,
                         "tap_bytes_requested": requested, "image_bytes_read_plus_written": 6 * B * H * W}
        print("%-30s warp %.4f ms (%.0f GB/s)  augment %.4f ms  clone %.4f ms (%.0f GB/s)  warp/clone %.2f  "
              "warp/augment %.2f" % (name, w, mb / w, a, c, mb / c, w / c, w / a), flush=True)
    print(json.dumps({"tool": "warp_bench", "device": torch.cuda.get_device_name(0), "batch": B, "height": H,
                      "width": W, "windows": args.windows, "window_ms": args.window_ms, "cases": results}))


if __name__ == "__main__":
    main()
