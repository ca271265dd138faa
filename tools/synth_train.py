#!/usr/bin/env python3
"""End-to-end accuracy record on procedural cable scenes: R18-8s and R34-8s trained from
the seeded initialisation on CableScenes at 640x480, B = 8, for `--steps` optimizer steps
(hkp.train.Trainer, FusedAdam, the reference's lr 1e-4 and weight decay 1e-4, fresh scenes
every step through DeviceBatches), then evaluated with hkp.metrics.KeypointMetrics on
`--held-out` fixed scenes of seed + 1 that training never sees.

Runs: loss "bce", and "qfl" with norm="instances"; absent="zero"; each with and without
augment= (DomainRandomization).  Evaluation follows train.py's eval_forward: one forward
per batch under no_grad (BN in training mode, as the reference's test loop), peaks decoded
from the low-res logits (max_peaks = instances, radius 1, threshold 0.1).

One JSON line per configuration: recall at 2 / 4 / 8 / 16 px per class, mAP, mean
localisation error, the mean train loss of the last 20 steps, images per second of the
training loop (host scene sampling included).  A record, not a gate."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "hulk-keypoints_amd"))

import torch  # noqa: E402


def train_model(backbone, loss, augment, args, dev):
    """The training half of a run: (model, scenes, held-out scenes, seconds, the mean
    train loss of the last 20 steps)."""
    from hkp import train
    from hkp.augment import DomainRandomization
    from hkp.synth import CableScenes
    from oracle import recipe
    from src.dataset import DeviceBatches, SynthDataset
    from src.model import KeypointsGauss
    hw, B = (args.height, args.width), args.batch
    scenes, held = CableScenes(seed=args.seed), CableScenes(seed=args.seed + 1)
    K = len(scenes.classes)
    model = KeypointsGauss(K, hw[0], hw[1], backbone=backbone, pretrained=False)
    model.load_state_dict(recipe.seeded_state_dict(backbone, 23))
    model = model.to(dev)
    params = {"beta": 2.0, "norm": "instances"} if loss == "qfl" else None
    tr = train.Trainer(model, lr=args.lr, loss=loss, absent="zero", loss_params=params)
    batches = DeviceBatches(SynthDataset(scenes, B * args.steps, hw, device=dev), B, device=dev,
                            augment=DomainRandomization(seed=args.seed) if augment else None)
    losses = []
    torch.cuda.synchronize()
    t0 = time.time()
    for img, pts in batches:
        losses.append(tr.step(img, pts=pts))
    torch.cuda.synchronize()
    secs = time.time() - t0
    tail = torch.stack([v.detach().double().reshape(()) for v in losses[-20:]]).mean().item()
    return model, scenes, held, secs, tail


def run(backbone, loss, augment, args, dev):
    from hkp import net, ops
    from hkp.metrics import KeypointMetrics
    from src.dataset import DeviceBatches, SynthDataset
    model, scenes, held, secs, tail = train_model(backbone, loss, augment, args, dev)
    hw, B = (args.height, args.width), args.batch
    K, M = len(scenes.classes), scenes.instances
    metrics = KeypointMetrics(K, (2, 4, 8, 16), device=dev)
    test = DeviceBatches(SynthDataset(held, args.held_out, hw, fixed=True, device=dev), B, device=dev)
    with torch.no_grad():
        for img, pts in test:
            _, _, low = net.keypoints_forward(model.resnet.net, img, K, pol=model.policy, upsample=False)
            peaks, counts = ops.heat_peaks(low, hw[0], hw[1], max_peaks=M, radius=1, threshold=0.1)
            metrics.update(peaks, counts, pts)
    res = metrics.compute()
    return {"backbone": backbone, "loss": loss, "augment": bool(augment), "steps": args.steps, "batch": B,
            "lr": args.lr, "train_seconds": secs, "train_img_per_s": B * args.steps / secs, "final_train_loss": tail,
            "classes": list(scenes.classes),
            "recall": {c: r["recall"] for c, r in zip(scenes.classes, res["per_class"])},
            "instances": {c: r["instances"] for c, r in zip(scenes.classes, res["per_class"])},
            "absent_false_alarms": {c: r["absent_false_alarms"] for c, r in zip(scenes.classes, res["per_class"])},
            "mAP": res["overall"]["mAP"], "recall_pooled": res["overall"]["recall"],
            "mean_error_px": res["overall"]["mean_error_px"]}


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
        sys.exit("synth_train: no GPU (there is no CPU path)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    for backbone in args.backbones.split(","):
        for loss in args.losses.split(","):
            for augment in (False, True):
                print(json.dumps(dict(tool="synth_train", device=torch.cuda.get_device_name(0),
                                      **run(backbone, loss, augment, args, dev))), flush=True)


if __name__ == "__main__":
    main()
