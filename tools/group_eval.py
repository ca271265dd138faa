#!/usr/bin/env python3
"""Grouping record on procedural cable scenes: tools/synth_train.py's recipe (R18-8s from
the seeded initialisation, 640x480, B = 8, `--steps` optimizer steps of hkp.train.Trainer on
fresh scenes, the reference's lr 1e-4 and weight decay 1e-4) with cables=(2, 2) and
associative-embedding tags on ("cap", "tail") — slot m of both classes is cable m — then, on
`--held-out` fixed scenes of seed + 1: one forward per batch under no_grad over the fc rows
0..2K-1, the peaks of the heat channels (max_peaks = instances, radius 1, threshold 0.1)
matched to the labels at 8 px (ops.peaks_match), grouped by tag (ops.peaks_group) and scored
with hkp.grouping.pair_scores: the share of cables with both ends matched whose cap and tail
carry one group id, and the share of predicted groups that mix two cables.

The comparison figure is 0.5: what pairing two caps with two tails at random gives.  One
JSON line with both shares, the held-out tag loss before and after training, the recall at
8 px and the mean train tag loss of the last 20 steps.  A record of one run, not a gate and
not a claim."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "hulk-keypoints_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--held-out", type=int, default=256)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--backbone", default="resnet18")
    ap.add_argument("--weight", type=float, default=1e-3)
    ap.add_argument("--max-dist", type=float, default=1.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("group_eval: no GPU (there is no CPU path)")
    from hkp import net, ops, train
    from hkp.grouping import pair_scores, slot_groups
    from hkp.metrics import KeypointMetrics
    from hkp.synth import CableScenes
    from oracle import recipe
    from src.dataset import DeviceBatches, SynthDataset
    from src.model import KeypointsGauss
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    hw, B = (args.height, args.width), args.batch
    scenes, held = CableScenes(seed=args.seed, cables=(2, 2)), CableScenes(seed=args.seed + 1, cables=(2, 2))
    names = list(scenes.classes)
    K, M = len(names), scenes.instances
    classes = (names.index("cap"), names.index("tail"))
    model = KeypointsGauss(K, hw[0], hw[1], backbone=args.backbone, pretrained=False)
    model.load_state_dict(recipe.seeded_state_dict(args.backbone, 23))
    model = model.to(dev)
    test = DeviceBatches(SynthDataset(held, args.held_out, hw, fixed=True, device=dev), B, device=dev)

    def held_out(score):
        """Mean tag loss (total, pull, push) over the held-out batches; with score=True also the
        grouping shares and the recall at 8 px."""
        metrics = KeypointMetrics(K, (8,), device=dev)
        acc, n = torch.zeros(3, device=dev, dtype=torch.float64), 0
        groups, matches, gids = [], [], []
        with torch.no_grad():
            for img, pts in test:
                low_all = net.keypoints_forward(model.resnet.net, img, K, pol=model.policy, upsample=False,
                                                tags=True)[2]
                gid = slot_groups(pts.shape[0], K, M, classes, dev)
                acc += ops.tag_loss(low_all, pts, gid, hw[0], hw[1], 1.0, want_grad=False)[0] * pts.shape[0]
                n += pts.shape[0]
                if score:
                    peaks, counts = ops.heat_peaks(low_all[:, :K].contiguous(), hw[0], hw[1], max_peaks=M, radius=1,
                                                   threshold=0.1)
                    _, gm, _ = ops.peaks_match(peaks, counts, pts, (8,), metrics.hist, metrics.totals,
                                               bins=metrics.bins, outputs=True)
                    group = ops.peaks_group(peaks, counts, low_all, hw[0], hw[1], classes, max_dist=args.max_dist)[0]
                    groups.append(group.cpu().numpy()), matches.append(gm.cpu().numpy()), gids.append(gid.cpu().numpy())
        out = {"tag_loss": (acc / n).tolist()}
        if score:
            out["pairs"] = pair_scores(np.concatenate(groups), np.concatenate(matches), np.concatenate(gids))
            res = metrics.compute()
            out["recall_8px"] = {c: r["recall"][0] for c, r in zip(names, res["per_class"])}
        return out

    before = held_out(False)
    tr = train.Trainer(model, lr=args.lr, loss="bce", absent="zero",
                       tags={"classes": classes, "weight": args.weight})
    tag_losses = []
    torch.cuda.synchronize()
    t0 = time.time()
    for img, pts in DeviceBatches(SynthDataset(scenes, B * args.steps, hw, device=dev), B, device=dev):
        tr.step(img, pts=pts)
        tag_losses.append(tr.tag_loss)
    torch.cuda.synchronize()
    secs = time.time() - t0
    after = held_out(True)
    print(json.dumps({"tool": "group_eval", "device": torch.cuda.get_device_name(0), "backbone": args.backbone,
                      "steps": args.steps, "batch": B, "lr": args.lr, "weight": args.weight, "max_dist": args.max_dist,
                      "classes": names, "tags_on": [names[c] for c in classes], "held_out": args.held_out,
                      "train_seconds": secs, "train_img_per_s": B * args.steps / secs,
                      "final_train_tag_loss": torch.stack(tag_losses[-20:]).mean(0).tolist(),
                      "held_out_tag_loss_before": before["tag_loss"], "held_out_tag_loss_after": after["tag_loss"],
                      "pairs": after["pairs"], "random_pairing": 0.5, "recall_8px": after["recall_8px"]}), flush=True)


if __name__ == "__main__":
    main()
