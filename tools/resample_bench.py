#!/usr/bin/env python3
"""HIP-event time of the antialiased-resize launch (hkp_resample_u8) alone at B=32,
next to a clone() of its input, next to the non-antialiased warp resize
(ops.resize_u8's launch, hkp_warp_affine_u8 under a resize matrix) on the same
shapes, and next to the domain-randomisation launch (hkp_augment_u8, the sampled
reference programs) at the output size, which it sits beside in the data path —
all in the same process.

Per case: warm-up, then `--windows` windows of `--window-ms` of back-to-back
launches each (events around the window, launch count calibrated from the
warm-up), with clone, augment, warp-resize and resample windows alternating; the
median window gives the time per launch.  Cases: 1280x960 -> 640x480 bilinear and
lanczos (stretch), 1920x1080 -> 640x480 bilinear (fit).  Also printed per case:
the source bytes the kernel's loads request (from the axis tables: every row
group walks its vertical span once per output column) against the distinct
source bytes.  One image of every case is compared with Pillow first.  Prints one
line per case and a JSON summary; not a gate."""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "hulk-keypoints_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROWS_PER_THREAD = 8          # RS_R of csrc/resample.hip


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


def requested_bytes(plan, b=0):
    """Source bytes image b's loads request: per row group of ROWS_PER_THREAD output
    rows, (rows of its vertical span) x (sum of the columns' tap counts) x 3."""
    from hkp import resample
    r = plan.records[b]
    _, xb, _ = resample.table_parts(plan.tables[r.xtab:])
    _, yb, _ = resample.table_parts(plan.tables[r.ytab:])
    taps = int(xb[:, 1].sum())
    h = plan.hw[0]
    rows = 0
    for g0 in range(0, h, ROWS_PER_THREAD):              # row groups are aligned to the output, not the rectangle
        ys = [y - r.y0 for y in range(g0, min(g0 + ROWS_PER_THREAD, h)) if 0 <= y - r.y0 < r.hd]
        if ys:
            rows += int(max(yb[y, 0] + yb[y, 1] for y in ys) - min(yb[y, 0] for y in ys))
    return rows * taps * 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=300.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("resample_bench: no GPU (there is no CPU path to time)")
    from PIL import Image
    from hkp import _lib, augment, geometry, resample
    from oracle import recipe
    dev = torch.device("cuda", 0)
    B, H, W = args.batch, args.height, args.width
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731

    y = torch.from_numpy(recipe.seeded_images_u8(B, H, W, 5)).to(dev)       # the augmentation's input, at the output size
    out = torch.empty_like(y)
    aplan = augment.DomainRandomization(seed=0).plan(range(B), 0)
    progs, luts = aplan.device_arrays(dev)
    table = augment.TABLE.on(dev)

    def aug():
        _lib.call("hkp_augment_u8", B, H, W, P(y), P(out), aplan.programs, P(progs), P(luts), P(table), stream)

    cases = [("1280x960 bilinear", 960, 1280, "bilinear", "stretch"), ("1280x960 lanczos", 960, 1280, "lanczos", "stretch"),
             ("1920x1080 fit bilinear", 1080, 1920, "bilinear", "fit")]
    results = {}
    for name, hs, ws, filt, mode in cases:
        src = recipe.seeded_images_u8(2, hs, ws, 7)
        x = torch.from_numpy(np.concatenate([src] * (B // 2) + [src[:B % 2]])).to(dev)
        plan = resample.ResamplePlan([(hs, ws)] * B, (H, W), filter=filt, mode=mode, fill=(9, 9, 9))
        recs, tabs = plan.device_arrays(dev)
        wplan = geometry.WarpPlan([geometry.resize_matrix(hs, ws, H, W)] * B, (H, W), border="replicate")
        xf = wplan.device_array(dev)
        th = ctypes.c_void_p(plan.tables.ctypes.data)

        def clone():
            x.clone()

        def rs():
            _lib.call("hkp_resample_u8", B, P(x), plan.in_bytes, plan.records, P(recs), th, P(tabs), plan.tables.size,
                      H, W, P(out), stream)

        def wr():
            _lib.call("hkp_warp_affine_u8", B, hs, ws, P(x), H, W, P(out), wplan.xforms, P(xf), wplan.interp,
                      wplan.border, stream)

        rs()
        torch.cuda.synchronize()
        x0, y0, wd, hd = plan.rects[0]
        want = np.asarray(Image.fromarray(src[0], "RGB").resize((int(wd), int(hd)), getattr(Image, filt.upper()),
                                                                reducing_gap=None))
        got = out[0].cpu().numpy()
        if not np.array_equal(got[y0:y0 + hd, x0:x0 + wd], want):
            sys.exit("resample_bench: %s differs from Pillow" % name)

        fns = (clone, aug, wr, rs)
        for fn in fns:                                   # warm-up, and the calibration of the window length
            _window(fn, 10)
        iters = [max(10, int(args.window_ms / _window(fn, 20))) for fn in fns]
        times = tuple([] for _ in fns)
        for _ in range(args.windows):                    # alternating: all four see the same machine state
            for t, fn, n in zip(times, fns, iters):
                t.append(_window(fn, n))
        c, a, w, r = (_median(t) for t in times)
        req, distinct = requested_bytes(plan), hs * ws * 3
        moved = B * (distinct + H * W * 3) / 1e6         # MB read once + written once; / ms = GB/s
        results[name] = {"resample_ms": r, "warp_resize_ms": w, "augment_ms": a, "clone_ms": c,
                         "resample_over_clone": r / c, "resample_over_augment": r / a, "resample_over_warp_resize": r / w,
                         "resample_GBps": moved / r, "clone_GBps": 2 * B * distinct / 1e6 / c,
                         "spread": {k: [min(t), max(t)] for k, t in zip(("clone", "augment", "warp_resize", "resample"),
                                                                        times)},
                         "launches_per_window": iters, "source_bytes_requested_per_image": req,
                         "source_bytes_distinct_per_image": distinct, "requested_over_distinct": req / distinct}
        print("%-24s resample %.4f ms (%.0f GB/s)  warp-resize %.4f ms  augment %.4f ms  clone %.4f ms  "
              "resample/clone %.2f  resample/augment %.2f  requested/distinct %.2f"
              % (name, r, moved / r, w, a, c, r / c, r / a, req / distinct), flush=True)
    print(json.dumps({"tool": "resample_bench", "device": torch.cuda.get_device_name(0), "batch": B, "height": H,
                      "width": W, "windows": args.windows, "window_ms": args.window_ms, "cases": results}))


if __name__ == "__main__":
    main()
