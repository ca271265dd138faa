#!/usr/bin/env python3
"""HIP-event time of the cable-scene launch (hkp_synth_cables_u8) alone at B=32,
640x480, next to a clone() of a uint8 batch of the same size and to the
domain-randomisation launch (hkp_augment_u8, sampled reference programs) in the same
process.  The renderer writes 3 B/pixel and reads next to nothing, so a device copy
(3 read + 3 written) is a loose yardstick: the kernel is bound by its integer
arithmetic per covering piece, not by memory traffic.

Per case: warm-up, then `--windows` windows of `--window-ms` of back-to-back launches
each (events around the window, launch count calibrated from the warm-up), clone,
augment and render windows alternating; the median window gives the time per launch.
Cases: the default scenes of CableScenes(seed=0); pictures without a piece (the
background and the store skeleton); the worst case the ABI admits, 512 pieces per
image spread over the picture.  Prints one line per case and a JSON summary; not a
gate."""
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


def worst_case(B, H, W, seed=1, n=512):
    """512 pieces per image: short capsules of radius 4..8 px all over the picture."""
    from hkp.synth import SynthPlan
    rng = np.random.default_rng(seed)
    polys, radii, cols = [], [], []
    for _ in range(B):
        a = rng.uniform((0, 0), (W, H), (n, 2))
        d = rng.uniform(-24, 24, (n, 2))
        polys.append([np.stack([p, p + q]) for p, q in zip(a, d)])
        radii.append([float(r) for r in rng.uniform(4.0, 8.0, n)])
        cols.append([tuple(int(v) for v in c) for c in rng.integers(0, 256, (n, 3))])
    return SynthPlan.from_polylines((H, W), polys, radii, cols)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--window-ms", type=float, default=300.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("synth_bench: no GPU (there is no CPU path to time)")
    from hkp import _lib, augment
    from hkp.synth import CableScenes, SynthPlan
    dev = torch.device("cuda", 0)
    B, H, W = args.batch, args.height, args.width
    out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
    aug_out = torch.empty_like(out)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731
    aplan = augment.DomainRandomization(seed=0).plan(range(B), 0)
    progs, luts = aplan.device_arrays(dev)
    table = augment.TABLE.on(dev)

    cases = {
        "default scenes": CableScenes(seed=0).plan(range(B), 0, (H, W)),
        "no pieces": SynthPlan.from_polylines((H, W), [[]] * B, [[]] * B, [[]] * B),
        "512 pieces per image": worst_case(B, H, W),
    }

    def clone():
        out.clone()

    def aug():
        _lib.call("hkp_augment_u8", B, H, W, P(out), P(aug_out), aplan.programs, P(progs), P(luts), P(table), stream)

    results = {}
    for name, plan in cases.items():
        scenes, segs = plan.device_arrays(dev)
        pieces = [sc.seg_cnt for sc in plan.scenes]

        def launch():
            _lib.call("hkp_synth_cables_u8", B, H, W, P(out), plan.scenes, P(scenes), plan.segs, P(segs), plan.nsegs,
                      stream)

        torch.cuda.synchronize()
        for fn in (clone, aug, launch):                  # warm-up, and the calibration of the window length
            _window(fn, 20)
        n_it = {fn: max(20, int(args.window_ms / _window(fn, 50))) for fn in (clone, aug, launch)}
        ts = {clone: [], aug: [], launch: []}
        for _ in range(args.windows):                    # alternating: all see the same machine state
            for fn in (clone, aug, launch):
                ts[fn].append(_window(fn, n_it[fn]))
        c, a, s = _median(ts[clone]), _median(ts[aug]), _median(ts[launch])
        mpx = B * H * W / 1e6
        results[name] = {"synth_ms": s, "clone_ms": c, "augment_ms": a, "synth_over_clone": s / c,
                         "synth_Gpx_per_s": mpx / s, "pieces_per_image": [min(pieces), max(pieces)],
                         "synth_spread": [min(ts[launch]), max(ts[launch])],
                         "clone_spread": [min(ts[clone]), max(ts[clone])],
                         "augment_spread": [min(ts[aug]), max(ts[aug])],
                         "launches_per_window": [n_it[launch], n_it[clone], n_it[aug]]}
        print("%-22s synth %.4f ms (%.1f Gpx/s, %d..%d pieces)  clone %.4f ms  augment %.4f ms  synth/clone %.2f" % (
            name, s, mpx / s, min(pieces), max(pieces), c, a, s / c), flush=True)
    print(json.dumps({"tool": "synth_bench", "device": torch.cuda.get_device_name(0), "batch": B, "height": H,
                      "width": W, "windows": args.windows, "window_ms": args.window_ms, "cases": results}))


if __name__ == "__main__":
    main()
