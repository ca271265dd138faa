#!/usr/bin/env python3
"""HIP-event time of the optimizer step over R34-8s's parameter list (random
gradients), with and without gradient clipping and the weight EMA, all in one process:

  adam            hkp_adam_step                                        28 B/element
  clip            hkp_grad_norm + hkp_adam_step_ex(coef)               32 B/element
  clip_ema        hkp_grad_norm + hkp_adam_step_ex(coef, ema)          40 B/element
  fused_step      FusedAdam(max_grad_norm, ema_decay).step()           the same launches through Python
  torch_unfused   clip_grad_norm_ + FusedAdam.step() + _foreach_lerp_  what the options replace

The first three are back-to-back C-ABI calls on prebuilt tables (device time of the
launches); the last two go through Python, as a training step does, so they compare
with each other.  Warm-up, then `--windows` windows of about `--window-ms` each (events
around the window, call count calibrated from the warm-up), the variants alternating
so that all see the same machine state; the median window gives the time per step.
Before timing, the parameters and EMA after one step are compared with the unfused
torch chain on the same inputs (largest difference relative to the largest value;
torch takes its norm in fp32 and its coefficient as reciprocal times max_norm, so the
two coefficients may differ in the last bits).  Bytes are counted from the element count
(read p, g, m, v and write p, m, v; + the norm's read of g; + read and write of the EMA).
Prints one line and a JSON summary; not a gate."""
import argparse
import ctypes
import json
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "hulk-keypoints_amd"))

import torch  # noqa: E402

BYTES = {"adam": 28, "clip": 32, "clip_ema": 40, "fused_step": 40}


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
    ap.add_argument("--backbone", default="resnet34")
    ap.add_argument("--keypoints", type=int, default=4)
    ap.add_argument("--max-grad-norm", type=float, default=1.0)
    ap.add_argument("--ema-decay", type=float, default=0.999)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--window-ms", type=float, default=300.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("optim_bench: no GPU (there is no CPU path to time)")
    from hkp import _lib
    from hkp.optim import FusedAdam
    from src.model import KeypointsGauss
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    shapes = [tuple(p.shape) for p in KeypointsGauss(args.keypoints, backbone=args.backbone,
                                                     pretrained=False).parameters()]
    n_elem = sum(math.prod(s) for s in shapes)
    gen = torch.Generator().manual_seed(1)
    base = [torch.randn(s, generator=gen) * 0.05 for s in shapes]
    grad = [torch.randn(s, generator=gen) * 0.01 for s in shapes]
    lr, wd, b1, b2, eps, step = 1e-4, 1e-4, 0.9, 0.999, 1e-8, 10
    adam_args = (b2, 1.0 - b1, 1.0 - b2, eps, wd, -lr / (1.0 - b1 ** step), math.sqrt(1.0 - b2 ** step))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731

    def state():
        """p, g, m, v, ema of one variant and its launch table."""
        ts = {k: [t.to(dev) for t in src] for k, src in (("p", base), ("g", grad), ("e", base))}
        ts["m"] = [torch.zeros_like(t) for t in ts["p"]]
        ts["v"] = [torch.zeros_like(t) for t in ts["p"]]
        arr = (_lib.AdamTensor * len(shapes))()
        ema = (ctypes.c_void_p * len(shapes))()
        for i in range(len(shapes)):
            arr[i].param, arr[i].grad = ts["p"][i].data_ptr(), ts["g"][i].data_ptr()
            arr[i].exp_avg, arr[i].exp_avg_sq = ts["m"][i].data_ptr(), ts["v"][i].data_ptr()
            arr[i].n = ts["p"][i].numel()
            ema[i] = ts["e"][i].data_ptr()
        return ts, arr, ema

    n = len(shapes)
    s_adam, a_adam, _ = state()
    s_clip, a_clip, _ = state()
    s_ce, a_ce, e_ce = state()
    need = _lib.lib().hkp_grad_norm_partials(n, a_adam)
    ws = torch.empty(need, dtype=torch.float64, device=dev)
    out = torch.zeros(2, device=dev)
    coef = ctypes.c_void_p(out.data_ptr() + 4)
    omd = 1.0 - args.ema_decay

    def adam():
        _lib.call("hkp_adam_step", n, a_adam, *adam_args, stream)

    def clip():
        _lib.call("hkp_grad_norm", n, a_clip, args.max_grad_norm, P(ws), need, P(out), stream)
        _lib.call("hkp_adam_step_ex", n, a_clip, None, 0.0, coef, *adam_args, stream)

    def clip_ema():
        _lib.call("hkp_grad_norm", n, a_ce, args.max_grad_norm, P(ws), need, P(out), stream)
        _lib.call("hkp_adam_step_ex", n, a_ce, e_ce, omd, coef, *adam_args, stream)

    def params():
        ps = [torch.nn.Parameter(t.to(dev)) for t in base]
        for p, g in zip(ps, grad):
            p.grad = g.to(dev)
        return ps
    p_f, p_t = params(), params()
    o_f = FusedAdam(p_f, lr=lr, weight_decay=wd, max_grad_norm=args.max_grad_norm, ema_decay=args.ema_decay)
    o_t = FusedAdam(p_t, lr=lr, weight_decay=wd)
    e_t = [p.detach().clone() for p in p_t]
    d_t = [p.detach() for p in p_t]

    def torch_unfused():
        torch.nn.utils.clip_grad_norm_(p_t, args.max_grad_norm)
        o_t.step()
        torch._foreach_lerp_(e_t, d_t, omd)

    # one step of each chain on the same inputs
    o_f.step()
    torch_unfused()
    torch.cuda.synchronize()
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())     # noqa: E731
    diff_p = max(rel(a.detach(), b.detach()) for a, b in zip(p_f, p_t))
    diff_e = max(rel(o_f.state[a]["ema"], e) for a, e in zip(p_f, e_t))
    for p, g in zip(p_t, grad):                      # clip_grad_norm_ scaled them in place
        p.grad.copy_(g)
    names = ["adam", "clip", "clip_ema", "fused_step", "torch_unfused"]
    fns = [adam, clip, clip_ema, o_f.step, torch_unfused]
    for fn in fns:                                   # warm-up, and the calibration of the window length
        _window(fn, 20)
    iters = [max(20, int(args.window_ms / _window(fn, 50))) for fn in fns]
    times = [[] for _ in fns]
    for _ in range(args.windows):                    # alternating: all see the same machine state
        for t, fn, k in zip(times, fns, iters):
            t.append(_window(fn, k))
    med = [_median(t) for t in times]
    gbs = {k: BYTES[k] * n_elem / (m * 1e-3) / 1e9 for k, m in zip(names, med) if k in BYTES}
    print("  ".join("%s %.1f us" % (k, 1e3 * m) for k, m in zip(names, med)), flush=True)
    print(json.dumps({"tool": "optim_bench", "device": torch.cuda.get_device_name(0), "backbone": args.backbone,
                      "tensors": n, "elements": n_elem, "max_grad_norm": args.max_grad_norm,
                      "ema_decay": args.ema_decay, "windows": args.windows, "window_ms": args.window_ms,
                      "grad_norm": float(o_f.grad_norm), "clip_coef": float(o_f.clip_coef),
                      "max_rel_diff_vs_torch_chain": {"param": diff_p, "ema": diff_e},
                      "us": {k: 1e3 * m for k, m in zip(names, med)},
                      "bytes_per_element": BYTES, "achieved_gb_s": gbs,
                      "over_adam": {k: m / med[0] for k, m in zip(names[1:], med[1:])},
                      "spread_us": {k: [1e3 * min(t), 1e3 * max(t)] for k, t in zip(names, times)},
                      "spread_rel": {k: (max(t) - min(t)) / m for k, t, m in zip(names, times, med)},
                      "calls_per_window": iters}))


if __name__ == "__main__":
    main()
