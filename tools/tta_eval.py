#!/usr/bin/env python3
"""Accuracy record of test-time augmentation on procedural cable scenes: the training
runs of tools/synth_train.py (R18-8s and R34-8s, "bce" and "qfl" with norm="instances",
no colour augmentation, `--steps` steps of B = 8 at 640x480 from the seeded
initialisation), then the same `--held-out` fixed scenes of seed + 1 scored with
KeypointsGauss.evaluate under

    tta=None | hflip | hflip + vflip | scales (0.75, 1, 1.25) + hflip

the last three in both merge modes ("prob", "logit").  BN stays in training mode, as in
the reference's test loop and synth_train: every view is a forward with its own batch
statistics.  Peaks: max_peaks = instances, radius 1, threshold 0.1.  The four classes
(cap, tail, crossing, blob) have no left / right pairs: flip_pairs is empty.

One JSON line per row: pooled recall at 2 / 4 / 8 / 16 px, crossing recall, mAP, mean
error, false alarms on absent planes (all classes, and the crossing planes alone).  A
record, not a gate: one training run per model and loss."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "hulk-keypoints_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import torch  # noqa: E402

VIEW_SETS = [("none", None), ("hflip", dict(hflip=True)), ("hflip+vflip", dict(hflip=True, vflip=True)),
             ("scales+hflip", dict(hflip=True, scales=(0.75, 1.0, 1.25)))]


def score(model, held, args, dev, tta):
    from hkp.metrics import KeypointMetrics
    from src.dataset import DeviceBatches, SynthDataset
    hw, B = (args.height, args.width), args.batch
    metrics = KeypointMetrics(len(held.classes), (2, 4, 8, 16), device=dev)
    for img, pts in DeviceBatches(SynthDataset(held, args.held_out, hw, fixed=True, device=dev), B, device=dev):
        model.evaluate(img, pts, metrics, max_peaks=held.instances, radius=1, threshold=0.1, tta=tta)
    res = metrics.compute()
    cross = res["per_class"][list(held.classes).index("crossing")]
    return {"recall_pooled": res["overall"]["recall"], "crossing_recall": cross["recall"], "mAP": res["overall"]["mAP"],
            "mean_error_px": res["overall"]["mean_error_px"],
            "absent_false_alarms": res["overall"]["absent_false_alarms"],
            "crossing_absent_false_alarms": cross["absent_false_alarms"], "peaks": res["overall"]["peaks"],
            "instances": res["overall"]["instances"]}


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
    ap.add_argument("--losses", default="bce,qfl")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tta_eval: no GPU (there is no CPU path)")
    import synth_train
    from hkp.tta import TestTimeAugmentation
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    for backbone in args.backbones.split(","):
        for loss in args.losses.split(","):
            model, scenes, held, secs, tail = synth_train.train_model(backbone, loss, False, args, dev)
            for name, kw in VIEW_SETS:
                for mode in (("prob", "logit") if kw else (None,)):
                    tta = TestTimeAugmentation(mode=mode, **kw) if kw else None
                    row = score(model, held, args, dev, tta)
                    print(json.dumps(dict(tool="tta_eval", device=torch.cuda.get_device_name(0), backbone=backbone,
                                          loss=loss, steps=args.steps, views=name, n_views=tta.n_views if tta else 1,
                                          mode=mode, final_train_loss=tail, **row)), flush=True)


if __name__ == "__main__":
    main()
