#!/usr/bin/env python3
"""What associative-embedding tags cost, in one process:

  * HIP-event time of the two launches alone — hkp_tag_loss (M = 4 label slots, gradient
    on) and hkp_peaks_group (P = 4, Q = 2) — at B = 8 and 32, K = 4 on the 60x80 lattice of a
    640x480 picture, next to hkp_heat_peaks (radius 1, max_peaks 4) on the same logits and
    the BCE loss launch of the same batch (hkp_heat_loss_multi on [B,4,480,640]).
  * A training step of R34-8s at 640x480, B = 8 (hkp.train.Trainer, FusedAdam), with
    tags=None and with tags on classes (0, 1): the head at 8 rows instead of 4 plus the
    two small launches (hkp_tag_loss and the concatenation of dtag).

Warm-up, then `--windows` windows of back-to-back calls each (events around the window),
the candidates alternating so that all see the same machine state; the median window
gives the time per call.  The loss launch is compared with the numpy restatement
(tests/_tags_ref.py) on the first two images first.  Prints one line per part and a JSON
summary; a record, not a gate."""
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


def launches(args, dev):
    import _tags_ref as ref
    from hkp import _lib
    K, M, Pk, H, W = 4, 4, 4, args.height, args.width
    h, w = H // 8, W // 8
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731
    names, fns, keep = [], [], []
    for B in (8, 32):
        rng = np.random.default_rng(B)
        low_np = rng.normal(0, 1, (B, 2 * K, h, w)).astype(np.float32)
        pts_np = np.zeros((B, K, M, 3), np.float32)
        pts_np[..., 0], pts_np[..., 1] = rng.uniform(0, W - 1, (B, K, M)), rng.uniform(0, H - 1, (B, K, M))
        pts_np[:, :, :2, 2] = 1                                     # two cables per picture
        gid_np = np.tile(np.arange(M, dtype=np.int32), (B, K, 1))
        low, pts, gid = (torch.from_numpy(a).to(dev) for a in (low_np, pts_np, gid_np))
        tags = ctypes.c_void_p(low.data_ptr() + 4 * K * h * w)
        out3 = torch.empty(3, device=dev, dtype=torch.float64)
        dtag = torch.empty((B, K, h, w), device=dev)
        ws = torch.empty(2 * B, device=dev, dtype=torch.float64)
        heat_low = low[:, :K].contiguous()
        peaks = torch.empty((B, K, Pk, 3), device=dev)
        counts = torch.empty((B, K), device=dev, dtype=torch.int32)
        tag = torch.empty((B, K, Pk), device=dev)
        group = torch.empty((B, K, Pk), device=dev, dtype=torch.int32)
        ng = torch.empty(B, device=dev, dtype=torch.int32)
        order = (ctypes.c_int32 * 2)(0, 1)
        heat = torch.sigmoid(torch.from_numpy(rng.normal(-3, 1, (B, K, H, W)).astype(np.float32)).to(dev))
        dheat = torch.empty_like(heat)
        loss = torch.empty((), device=dev, dtype=torch.float64)
        lws = torch.empty(_lib.lib().hkp_heat_loss_multi_workspace(B, K, H, W) // 8, device=dev, dtype=torch.float64)
        keep.append((low, pts, gid, out3, dtag, ws, heat_low, peaks, counts, tag, group, ng, order, heat, dheat, loss, lws))

        def f_loss(B=B, tags=tags, pts=pts, gid=gid, out3=out3, dtag=dtag, ws=ws):
            return lambda: _lib.call("hkp_tag_loss", B, K, M, h, w, H, W, tags, 2 * K * h * w, P(pts), P(gid), 1e-3, 1.0,
                                     1.0, P(out3), P(dtag), P(ws), stream)

        def f_peaks(B=B, heat_low=heat_low, peaks=peaks, counts=counts):
            return lambda: _lib.call("hkp_heat_peaks", B, K, h, w, H, W, 1, Pk, 0.0, P(heat_low), P(peaks), P(counts),
                                     stream)

        def f_group(B=B, tags=tags, peaks=peaks, counts=counts, tag=tag, group=group, ng=ng, order=order):
            return lambda: _lib.call("hkp_peaks_group", B, K, Pk, h, w, H, W, 2, order, 1.0, P(peaks), P(counts), tags,
                                     2 * K * h * w, P(tag), P(group), P(ng), stream)

        def f_bce(B=B, heat=heat, pts=pts, loss=loss, dheat=dheat, lws=lws):
            return lambda: _lib.call("hkp_heat_loss_multi", B, K, M, H, W, 0, 0, P(heat), P(pts), 8.0, P(loss), P(dheat),
                                     P(lws), stream)

        f_loss()()
        torch.cuda.synchronize()
        r_out, r_dtag = ref.tag_loss(low_np[:2, K:], pts_np[:2], gid_np[:2], H, W, 1e-3 * 2 / B)
        if not np.allclose(dtag[:2].cpu().numpy(), r_dtag, rtol=1e-5, atol=1e-12):
            sys.exit("tags_bench: hkp_tag_loss differs from the restatement (B %d)" % B)
        f_peaks()()
        names += ["tag_loss_b%d" % B, "peaks_group_b%d" % B, "heat_peaks_b%d" % B, "bce_loss_b%d" % B]
        fns += [f_loss(), f_group(), f_peaks(), f_bce()]
    times = _alternate(fns, args.windows, args.window_ms)
    med = {k: 1e3 * _median(t) for k, t in zip(names, times)}
    print("  ".join("%s %.2f us" % kv for kv in med.items()), flush=True)
    return {"us": med, "spread_us": {k: [1e3 * min(t), 1e3 * max(t)] for k, t in zip(names, times)}}


def steps(args, dev):
    from hkp import train
    from hkp.synth import CableScenes
    from oracle import recipe
    from src.dataset import DeviceBatches, SynthDataset
    from src.model import KeypointsGauss
    hw, B = (args.height, args.width), 8
    scenes = CableScenes(seed=3, cables=(2, 2))
    K = len(scenes.classes)
    img, pts = next(iter(DeviceBatches(SynthDataset(scenes, B, hw, fixed=True, device=dev), B, device=dev)))
    fns = []
    for tags in (None, {"classes": (0, 1)}):
        model = KeypointsGauss(K, hw[0], hw[1], backbone=args.backbone, pretrained=False)
        model.load_state_dict(recipe.seeded_state_dict(args.backbone, 23))
        tr = train.Trainer(model.to(dev), tags=tags)
        fns.append(lambda tr=tr: tr.step(img, pts=pts))
    times = _alternate(fns, args.windows, args.window_ms * 5, floor=5)
    med = {k: _median(t) for k, t in zip(("step_plain_ms", "step_tags_ms"), times)}
    med["tags_over_plain"] = med["step_tags_ms"] / med["step_plain_ms"]
    print("  ".join("%s %.3f" % kv for kv in med.items()), flush=True)
    return {"backbone": args.backbone, "batch": B, "ms": med,
            "spread_ms": {k: [min(t), max(t)] for k, t in zip(("step_plain_ms", "step_tags_ms"), times)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--backbone", default="resnet34")
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--window-ms", type=float, default=100.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tags_bench: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    out = {"tool": "tags_bench", "device": torch.cuda.get_device_name(0), "height": args.height, "width": args.width,
           "windows": args.windows, "launches": launches(args, dev), "train_step": steps(args, dev)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
