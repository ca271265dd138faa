#!/usr/bin/env python3
"""Does a centreline plane help the point classes?  tools/synth_train.py's recipe (R18-8s
and R34-8s from the seeded initialisation, CableScenes at 640x480, B = 8, `--steps`
Trainer steps with BCE on fresh scenes, FusedAdam at lr 1e-4) with the classes (cap, tail,
crossing, blob, cable) against (cap, tail, crossing, blob): the same scenes, the extra
plane trained against hkp_line_target of the cables' pieces (Trainer.step(img, pts=pts,
lines=lines)).

Evaluated on `--held-out` fixed scenes of seed + 1: the four point classes with
hkp.metrics.KeypointMetrics exactly as synth_train does (peaks of the low-res logits,
max_peaks = instances, radius 1, threshold 0.1), and the cable plane with
hkp.lines.LineMetrics (radius 4 px, threshold 0.5) on the full-size heatmap.  One JSON line
per run, appended to --log; one run each: a record, not a gate.

--lines walk trains the cable plane through hkp_heat_loss_lines (Trainer(loss_params={"lines":
"walk"})) instead of the dense target; with it --loss qfl --beta 2 is possible.  --cable-only
skips the runs without the cable plane."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "hulk-keypoints_amd"))

import torch  # noqa: E402

POINTS = ("cap", "tail", "crossing", "blob")


def run(backbone, with_cable, args, dev):
    from hkp import net, ops, train
    from hkp.lines import LineMetrics
    from hkp.metrics import KeypointMetrics
    from hkp.synth import CableScenes
    from oracle import recipe
    from src.dataset import DeviceBatches, SynthDataset
    from src.model import KeypointsGauss
    hw, B = (args.height, args.width), args.batch
    classes = POINTS + (("cable",) if with_cable else ())
    scenes, held = CableScenes(seed=args.seed, classes=classes), CableScenes(seed=args.seed + 1, classes=classes)
    K, KP, M = len(classes), len(POINTS), scenes.instances
    model = KeypointsGauss(K, hw[0], hw[1], backbone=backbone, pretrained=False)
    model.load_state_dict(recipe.seeded_state_dict(backbone, 23))
    model = model.to(dev)
    params = {"lines": args.lines} if with_cable else {}
    if args.loss == "qfl":
        params["beta"] = args.beta
    tr = train.Trainer(model, lr=args.lr, loss=args.loss, absent="zero", loss_params=params)
    losses = []
    torch.cuda.synchronize()
    t0 = time.time()
    for batch in DeviceBatches(SynthDataset(scenes, B * args.steps, hw, device=dev), B, device=dev):
        if with_cable:
            losses.append(tr.step(batch[0], pts=batch[1], lines=batch[2]))
        else:
            losses.append(tr.step(batch[0], pts=batch[1]))
    torch.cuda.synchronize()
    secs = time.time() - t0
    metrics = KeypointMetrics(KP, (2, 4, 8, 16), device=dev)
    lm = LineMetrics(K, radius=4.0, threshold=0.5) if with_cable else None
    with torch.no_grad():
        for batch in DeviceBatches(SynthDataset(held, args.held_out, hw, fixed=True, device=dev), B, device=dev):
            img, pts = batch[0], batch[1]
            hm, _, low = net.keypoints_forward(model.resnet.net, img, K, pol=model.policy, upsample=with_cable)
            peaks, counts = ops.heat_peaks(low[:, :KP].contiguous(), hw[0], hw[1], max_peaks=M, radius=1, threshold=0.1)
            metrics.update(peaks, counts, pts[:, :KP].contiguous())
            if with_cable:
                lm.update(hm, batch[2])
    res = metrics.compute()
    out = {"backbone": backbone, "classes": list(classes), "steps": args.steps, "batch": B, "lr": args.lr,
           "loss": args.loss, "beta": args.beta if args.loss == "qfl" else None,
           "lines": args.lines if with_cable else None, "train_seconds": secs, "train_img_per_s": B * args.steps / secs,
           "final_train_loss": torch.stack([v.detach().double().reshape(()) for v in losses[-20:]]).mean().item(),
           "recall": {c: r["recall"] for c, r in zip(POINTS, res["per_class"])},
           "instances": {c: r["instances"] for c, r in zip(POINTS, res["per_class"])},
           "mAP": res["overall"]["mAP"], "recall_pooled": res["overall"]["recall"],
           "mean_error_px": res["overall"]["mean_error_px"]}
    if with_cable:
        out["cable_line_metrics"] = lm.compute()[K - 1]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--held-out", type=int, default=256)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--backbones", default="resnet18,resnet34")
    ap.add_argument("--loss", default="bce", choices=("bce", "mse", "qfl"))
    ap.add_argument("--beta", type=float, default=2.0)
    ap.add_argument("--lines", default="dense", choices=("dense", "walk"))
    ap.add_argument("--cable-only", action="store_true")
    ap.add_argument("--log", default=os.path.join(REPO, "profiles", "lines_eval.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lines_eval: no GPU (there is no CPU path)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    for backbone in args.backbones.split(","):
        for with_cable in ((True,) if args.cable_only else (False, True)):
            line = json.dumps(dict(tool="lines_eval", device=torch.cuda.get_device_name(0),
                                   **run(backbone, with_cable, args, dev)))
            print(line, flush=True)
            with open(args.log, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
