#!/usr/bin/env python3
"""Write procedural cable scenes to disk in the reference's directory layout:

    DIR/train/images/%05d.jpg   DIR/train/keypoints/%05d.npy
    DIR/test/images/%05d.jpg    DIR/test/keypoints/%05d.npy

N train scenes of CableScenes(seed) (epoch 0) and max(N // 4, 1) test scenes of seed + 1
(what config.SYNTH's fixed test set draws), rendered on the GPU (hkp_synth_cables_u8) and
saved as JPEG (quality 95) through Pillow; labels are float32 [K, M, 3] (u, v, flag), the
format KeypointsDataset(instances=M) reads, so the file path of this project and the
reference itself (which takes [K, 2]: pass --classes cap,tail --cables 1 --first-only)
can train on the same scenes.  JPEG is lossy: the files are not the rendered bits."""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "hulk-keypoints_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("n", type=int)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--classes", default="cap,tail,crossing,blob")
    ap.add_argument("--cables", type=int, default=None, help="exactly this many cables per scene (default 1..2)")
    ap.add_argument("--instances", type=int, default=8)
    ap.add_argument("--first-only", action="store_true",
                    help="labels [K, 2]: the first instance of every class (needs classes that are always present)")
    ap.add_argument("--batch", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("synth_export: no GPU (the scenes are rendered by hkp_synth_cables_u8; there is no CPU path)")
    from PIL import Image
    from hkp import ops
    from hkp.synth import CableScenes
    kw = {"classes": tuple(args.classes.split(",")), "instances": args.instances}
    if args.cables is not None:
        kw["cables"] = (args.cables, args.cables)
    hw = (args.height, args.width)
    for split, seed, n in (("train", args.seed, args.n), ("test", args.seed + 1, max(args.n // 4, 1))):
        scenes = CableScenes(seed=seed, **kw)
        img_dir, kp_dir = os.path.join(args.dir, split, "images"), os.path.join(args.dir, split, "keypoints")
        os.makedirs(img_dir, exist_ok=True)
        os.makedirs(kp_dir, exist_ok=True)
        for i0 in range(0, n, args.batch):
            idx = range(i0, min(i0 + args.batch, n))
            plan = scenes.plan(idx, 0, hw)
            imgs = ops.synth_cables_u8(plan).cpu().numpy()
            for b, i in enumerate(idx):
                Image.fromarray(np.ascontiguousarray(imgs[b][:, :, ::-1])).save(
                    os.path.join(img_dir, "%05d.jpg" % i), format="JPEG", quality=95)
                pts = plan.pts[b]
                if args.first_only:
                    if not (pts[:, 0, 2] > 0).all():
                        sys.exit("synth_export: --first-only, but scene %d of %s lacks a class" % (i, split))
                    pts = pts[:, 0, :2]
                np.save(os.path.join(kp_dir, "%05d.npy" % i), pts)
        print("%s: %d scenes -> %s" % (split, n, os.path.join(args.dir, split)))


if __name__ == "__main__":
    main()
