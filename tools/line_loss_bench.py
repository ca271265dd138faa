#!/usr/bin/env python3
"""What a line plane costs in the loss, in one process: HIP-event time at B = 8, K = 4,
480x640, sigma = 8, three point planes and one line plane of 96 present segments
(tools/lines_bench.py's mixed shape), of

  * the dense chain, hkp_line_target (fp64 target stored) + hkp_heat_loss (BCE, with dheat):
    what a line plane trains through under the defaults;
  * hkp_heat_loss_lines, the target in registers, in five forms: BCE, "qfl" at beta = 2, BCE
    with plane weights, BCE with a 30 % mask, BCE with topk = 2 (two passes);
  * hkp_heat_loss_planes (BCE) on four point planes: the floor, the same bytes without a
    segment loop.

Warm-up, then `--windows` windows of `--window-ms` of back-to-back calls each (events around
the window), the candidates alternating so that all see the same machine state; the median
window gives the time per call.  Before timing, dheat of the new entry is compared bit for
bit with the dense chain's.  Prints one line per candidate with its window-to-window spread
and a JSON summary, and appends both to --log; a record, not a gate."""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "hulk-keypoints_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from lines_bench import _alternate, _median, scene_lines  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--log", default=os.path.join(REPO, "profiles", "line_loss_bench.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("line_loss_bench: no GPU (there is no CPU path to time)")
    from hkp import _lib
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, K, S, H, W = args.batch, 4, 96, args.height, args.width
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())     # noqa: E731
    rng = np.random.default_rng(2)
    g = torch.Generator().manual_seed(3)

    l96 = scene_lines(B, (H, W), 2)
    assert (l96[..., 4] > 0).sum() == 96 * B
    k4 = np.zeros((B, K, S, 5), dtype=np.float32)
    uv = rng.uniform(0, [W - 1, H - 1], (B, 3, 2)).astype(np.float32)
    k4[:, :3, 0, 0:2], k4[:, :3, 0, 2:4], k4[:, :3, 0, 4] = uv, uv, 1.0
    k4[:, 3] = l96[:, 0]
    lines = torch.from_numpy(k4).to(dev)
    pts_np = np.zeros((B, K, 1, 3), dtype=np.float32)
    pts_np[..., 0, 0:2] = rng.uniform(0, [W - 1, H - 1], (B, K, 2))
    pts_np[..., 2] = 1.0
    pts = torch.from_numpy(pts_np).to(dev)
    heat = (torch.rand(B, K, H, W, generator=g) * 0.98 + 0.01).to(dev)
    weights = (torch.rand(B, K, generator=g) + 0.5).to(dev)
    mask = torch.zeros(B, H, W, dtype=torch.int64)
    for c in range(K):
        mask |= (torch.rand(B, H, W, generator=g) < 0.3).long() << c
    mask = mask.to(torch.uint8).to(dev)

    L = _lib.lib()
    f64 = lambda nbytes: torch.empty(nbytes // 8, device=dev, dtype=torch.float64)     # noqa: E731
    target = torch.empty((B, K, H, W), device=dev, dtype=torch.float64)
    dheat, dheat_ref = torch.empty_like(heat), torch.empty_like(heat)
    loss = torch.zeros((), device=dev, dtype=torch.float64)
    ws_dense, ws_planes = f64(L.hkp_heat_loss_workspace()), f64(L.hkp_heat_loss_planes_workspace(B, K, H, W))
    ws_lines = f64(L.hkp_heat_loss_lines_workspace(B, K, H, W))
    BCE, QFL = _lib.HKP_LOSS_BCE, _lib.HKP_LOSS_QFL

    def dense():
        _lib.call("hkp_line_target", B, K, S, H, W, 8.0, P(lines), P(target), None, stream)
        _lib.call("hkp_heat_loss", B, K, H, W, BCE, P(heat), P(target), None, 8.0, P(loss), P(dheat_ref), P(ws_dense),
                  stream)

    def walk(kind=BCE, w=None, m=None, topk=0):
        _lib.call("hkp_heat_loss_lines", B, K, S, H, W, kind, 0, 0, 2.0, topk, P(heat), P(lines), P(w), P(m), 8.0, P(loss),
                  P(dheat), None, None, None, P(ws_lines), stream)

    def planes():
        _lib.call("hkp_heat_loss_planes", B, K, 1, H, W, BCE, 0, 0, 2.0, 0, P(heat), P(pts), None, 8.0, P(loss), P(dheat),
                  None, None, P(ws_planes), stream)

    dense()
    walk()
    torch.cuda.synchronize()
    if not torch.equal(dheat.view(torch.int32), dheat_ref.view(torch.int32)):
        sys.exit("line_loss_bench: hkp_heat_loss_lines' dheat differs from the dense chain's")
    cands = [("dense_chain_bce", dense), ("lines_bce", walk), ("lines_qfl_beta2", lambda: walk(QFL)),
             ("lines_bce_weights", lambda: walk(w=weights)), ("lines_bce_mask30", lambda: walk(m=mask)),
             ("lines_bce_topk2", lambda: walk(topk=2)), ("planes_bce_4_point_planes", planes)]
    names, fns = [c[0] for c in cands], [c[1] for c in cands]
    times = _alternate(fns, args.windows, args.window_ms)
    med = {k: 1e3 * _median(t) for k, t in zip(names, times)}
    lines_out = ["%-28s %9.2f us  (%.2f .. %.2f)" % (k, med[k], 1e3 * min(t), 1e3 * max(t)) for k, t in zip(names, times)]
    spread = {k: [1e3 * min(t), 1e3 * max(t)] for k, t in zip(names, times)}
    gain = med["dense_chain_bce"] - med["lines_bce"]
    noise = (spread["dense_chain_bce"][1] - spread["dense_chain_bce"][0]) + (spread["lines_bce"][1] - spread["lines_bce"][0])
    lines_out.append("dense chain - lines (BCE): %.2f us, window-to-window spread of the two together %.2f us: %s"
                     % (gain, noise, "faster" if gain > noise else "NOT faster beyond the spread"))
    out = {"tool": "line_loss_bench", "device": torch.cuda.get_device_name(0), "batch": B, "classes": K, "height": H,
           "width": W, "segments": S, "windows": args.windows, "window_ms": args.window_ms, "us": med, "spread_us": spread,
           "bytes_per_pixel": {"dense_chain": 24, "lines": 8, "lines_mask": 8.25, "planes": 8}}
    text = "\n".join(lines_out + [json.dumps(out)])
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "a") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
