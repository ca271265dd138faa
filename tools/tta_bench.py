#!/usr/bin/env python3
"""HIP-event time of the test-time-augmentation merge (hkp_logits_merge) at the C2
decode shape, B=32, K=4, 60x80: the launch alone for 2 views (plain + hflip) and for
6 views (scales 1, 0.75, 1.25 x {plain, hflip}: lattices 60x80, 45x60, 75x100), in
both modes, and ops.logits_merge around it (the views' copies into the packed buffer
included), next to the hkp_heat_peaks launch (radius 1, max_peaks 4) on the merged
logits — all in the same process.  Then KeypointsGauss.predict_peaks on R34-8s
(seeded weights, uint8 640x480 batch) without TTA, with the flip view and with the 6
views: the ratio to one forward.

Warm-up, then `--windows` windows of `--window-ms` of back-to-back calls each (events
around the window, call count calibrated from the warm-up), alternating so that all
see the same machine state; the median window gives the time per call.  The merged
logits are compared with the numpy restatement (tests/_tta_ref.py) first.  Prints one
line per group and a JSON summary; not a gate."""
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


def measure(names, fns, windows, window_ms):
    for fn in fns:                                       # warm-up, and the calibration of the window length
        _window(fn, 5)
    iters = [max(5, int(window_ms / _window(fn, 10))) for fn in fns]
    times = [[] for _ in fns]
    for _ in range(windows):                             # alternating: all see the same machine state
        for t, fn, n in zip(times, fns, iters):
            t.append(_window(fn, n))
    return {k: {"us": 1e3 * _median(t), "spread_us": [1e3 * min(t), 1e3 * max(t)], "calls_per_window": n}
            for k, t, n in zip(names, times, iters)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--keypoints", type=int, default=4)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--backbone", default="resnet34")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tta_bench: no GPU (there is no CPU path to time)")
    import _tta_ref as ref
    from hkp import _lib, ops
    from hkp.tta import MODES, TestTimeAugmentation
    from oracle import recipe
    from src.model import KeypointsGauss
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, K, H, W = args.batch, args.keypoints, args.height, args.width
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731
    sets = {"2_views": TestTimeAugmentation(hflip=True),
            "6_views": TestTimeAugmentation(hflip=True, scales=(1.0, 0.75, 1.25))}
    rng = np.random.default_rng(1)
    names, fns, keep = [], [], []
    for sname, t in sets.items():
        plan = t.plan(B, K, H, W)
        h, w = plan.hw
        lows_np = [rng.normal(0, 2, (B, K) + lat).astype(np.float32) for lat in plan.lattices]
        lows = [torch.from_numpy(a).to(dev) for a in lows_np]
        packed = torch.cat([a.reshape(-1) for a in lows])
        table, perm = plan.device_arrays(dev)
        out = torch.empty((B, K, h, w), device=dev)
        for mode, code in MODES.items():
            got = ops.logits_merge(lows, plan, mode=mode).cpu().numpy()
            want = ref.merge([a[:2] for a in lows_np], plan.coefficients(), plan.perm, (h, w), code)
            if not ref.within_ulps(got[:2], want, 0 if mode == "logit" else 1):
                sys.exit("tta_bench: %s %s differs from the restatement" % (sname, mode))

            def launch(code=code, plan=plan, packed=packed, table=table, perm=perm, out=out, h=h, w=w):
                _lib.call("hkp_logits_merge", B, K, h, w, plan.n_views, code, P(packed), P(table), P(perm), P(out), stream)

            def wrapped(mode=mode, plan=plan, lows=lows, out=out):
                ops.logits_merge(lows, plan, mode=mode, out=out)
            names += ["merge_%s_%s" % (sname, mode), "ops_merge_%s_%s" % (sname, mode)]
            fns += [launch, wrapped]
        keep.append((lows, packed, table, perm, out))
    merged = keep[0][4]
    pk = torch.empty((B, K, 4, 3), device=dev)
    ct = torch.empty((B, K), device=dev, dtype=torch.int32)
    names.append("heat_peaks_r1_p4")
    fns.append(lambda: _lib.call("hkp_heat_peaks", B, K, H // 8, W // 8, H, W, 1, 4, 0.1, P(merged), P(pk), P(ct), stream))
    kern = measure(names, fns, args.windows, args.window_ms)
    print("  ".join("%s %.2f us" % (k, v["us"]) for k, v in kern.items()), flush=True)

    model = KeypointsGauss(K, H, W, backbone=args.backbone, pretrained=False)
    model.load_state_dict(recipe.seeded_state_dict(args.backbone, 3))
    model = model.to(dev)
    x = torch.from_numpy(recipe.seeded_images_u8(B, H, W, 5)).to(dev)
    cases = {"predict_peaks": None, "predict_peaks_flip": sets["2_views"], "predict_peaks_6_views": sets["6_views"]}
    e2e = measure(list(cases), [lambda t=t: model.predict_peaks(x, max_peaks=4, radius=1, threshold=0.1, tta=t)
                                for t in cases.values()], args.windows, args.window_ms)
    base = e2e["predict_peaks"]["us"]
    for k, v in e2e.items():
        v["over_one_forward"] = v["us"] / base
    print("  ".join("%s %.3f ms (x%.2f)" % (k, v["us"] / 1e3, v["over_one_forward"]) for k, v in e2e.items()), flush=True)
    print(json.dumps({"tool": "tta_bench", "device": torch.cuda.get_device_name(0), "batch": B, "keypoints": K,
                      "height": H, "width": W, "backbone": args.backbone, "windows": args.windows,
                      "window_ms": args.window_ms, "kernels": kern, "end_to_end": e2e}))


if __name__ == "__main__":
    main()
