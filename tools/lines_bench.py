#!/usr/bin/env python3
"""What the centreline target costs, in one process: HIP-event time of the hkp_line_target
launch at B = 8, 480x640, for

  * one line plane (K = 1) of 48 present segments and one of 96 (one and two cables of the
    default scenes, hkp.synth.CableScenes at 48 pieces a cable; the slots are S = 96);
  * K = 4 with three point planes (one zero-length segment each) and one line plane of 96;
  * each with the target alone, d2 alone, and both;

next to hkp_gauss_target_multi at M = 1 and M = 16 on the same shapes (M = 16 stores the
same bytes as the target and evaluates 16 exponentials a pixel) and a clone() of the fp64
target (the bytes alone, read and written).

Warm-up, then `--windows` windows of `--window-ms` of back-to-back calls each (events around
the window), the candidates alternating so that all see the same machine state; the median
window gives the time per call.  Before timing, d2 of the first image is compared with the
numpy restatement (tests/_lines_ref.py), which does not cull.  Prints one line per
candidate and a JSON summary, and appends both to --log; a record, not a gate."""
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


def _alternate(fns, windows, window_ms, floor=20):
    for fn in fns:
        _window(fn, 5)
    iters = [max(floor, int(window_ms / _window(fn, 10))) for fn in fns]
    times = [[] for _ in fns]
    for _ in range(windows):
        for t, fn, n in zip(times, fns, iters):
            t.append(_window(fn, n))
    return times


def scene_lines(B, hw, cables, seed=1):
    """float32 [B,1,96,5]: the cable plane of B default scenes with exactly `cables` cables."""
    from hkp.synth import CableScenes
    cs = CableScenes(seed=seed, classes=("cable",), cables=(cables, cables))
    plan = cs.plan(range(B), 0, hw)
    out = np.zeros((B, 1, 96, 5), dtype=np.float32)
    out[:, :, :plan.lines.shape[2]] = plan.lines
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--log", default=os.path.join(REPO, "profiles", "lines_bench.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lines_bench: no GPU (there is no CPU path to time)")
    import _lines_ref as ref
    from hkp import _lib
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, H, W = args.batch, args.height, args.width
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())     # noqa: E731
    rng = np.random.default_rng(2)

    l48, l96 = scene_lines(B, (H, W), 1), scene_lines(B, (H, W), 2)
    assert (l48[..., 4] > 0).sum() == 48 * B and (l96[..., 4] > 0).sum() == 96 * B
    k4 = np.zeros((B, 4, 96, 5), dtype=np.float32)
    uv = rng.uniform(0, [W - 1, H - 1], (B, 3, 2)).astype(np.float32)
    k4[:, :3, 0, 0:2], k4[:, :3, 0, 2:4], k4[:, :3, 0, 4] = uv, uv, 1.0
    k4[:, 3] = l96[:, 0]
    names, fns, keep = [], [], []
    for tag, lines_np in (("k1_s48", l48), ("k1_s96", l96), ("k4_3pts_s96", k4)):
        K = lines_np.shape[1]
        lines = torch.from_numpy(lines_np).to(dev)
        target = torch.empty((B, K, H, W), device=dev, dtype=torch.float64)
        d2 = torch.empty((B, K, H, W), device=dev, dtype=torch.float32)
        _lib.call("hkp_line_target", B, K, 96, H, W, 8.0, P(lines), P(target), P(d2), stream)
        torch.cuda.synchronize()
        if not np.array_equal(d2[0].cpu().numpy().view(np.uint32), ref.d2(lines_np[:1], H, W)[0].view(np.uint32)):
            sys.exit("lines_bench: hkp_line_target differs from the restatement (%s)" % tag)
        for what, t, d in (("target", target, None), ("d2", None, d2), ("both", target, d2)):
            names.append("line_target_%s_%s" % (tag, what))
            fns.append(lambda K=K, lines=lines, t=t, d=d: _lib.call("hkp_line_target", B, K, 96, H, W, 8.0, P(lines), P(t),
                                                                   P(d), stream))
        if tag == "k1_s96":                               # K = 1 comes twice: its comparisons once, above
            keep.append((lines, target, d2))
            continue
        for M in (1, 16):
            pts_np = np.zeros((B, K, M, 3), dtype=np.float32)
            pts_np[..., 0], pts_np[..., 1] = rng.uniform(0, W - 1, (B, K, M)), rng.uniform(0, H - 1, (B, K, M))
            pts_np[..., 2] = 1.0
            pts = torch.from_numpy(pts_np).to(dev)
            names.append("gauss_target_multi_k%d_m%d" % (K, M))
            fns.append(lambda K=K, M=M, pts=pts, target=target: _lib.call("hkp_gauss_target_multi", B, K, M, H, W, 8.0,
                                                                         P(pts), P(target), stream))
            keep.append(pts)
        names.append("clone_f64_k%d" % K)
        fns.append(lambda target=target: target.clone())
        keep.append((lines, target, d2))
    times = _alternate(fns, args.windows, args.window_ms)
    med = {k: 1e3 * _median(t) for k, t in zip(names, times)}
    lines_out = ["%-36s %9.2f us  (%.2f .. %.2f)" % (k, med[k], 1e3 * min(t), 1e3 * max(t)) for k, t in zip(names, times)]
    out = {"tool": "lines_bench", "device": torch.cuda.get_device_name(0), "batch": B, "height": H, "width": W,
           "windows": args.windows, "window_ms": args.window_ms, "us": med,
           "spread_us": {k: [1e3 * min(t), 1e3 * max(t)] for k, t in zip(names, times)},
           "stored_bytes": {"target_per_plane": 8 * H * W, "d2_per_plane": 4 * H * W}}
    text = "\n".join(lines_out + [json.dumps(out)])
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "a") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
