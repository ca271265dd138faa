"""analysis.py of the reference (analysis.py:1-43) on the MI355X path:
load a checkpoint (reference state_dict format), run every image of a folder
through Prediction, decode keypoints on the GPU and write the overlay grid.

    python analysis.py <checkpoint name under checkpoints/> <image dir>
    torchrun --nproc-per-node N analysis.py <ckpt> <image dir>      (data parallel)

Data parallel: each rank takes a contiguous slice of the sorted
file list (hkp.parallel.shard_range), writes its own overlays (preds/outNNNN.png,
NNNN = the image's index in the full list, as the single-GPU run names them),
and the int32 (y, x) keypoints of all images are all-gathered; rank 0 saves
them as preds/keypoints.npy ([n_images, K, 2], file order).  Images go through
one at a time (batch 1, train-mode BN — analysis.py:36-42), so results do not
depend on the GPU count.

With config.RESIZE set, an image whose size differs from the model's is resampled
on the GPU first (antialiased, hkp.resample.Resize(RESIZE, **RESIZE_PARAMS)); its
row of keypoints.npy then holds the predictions mapped back into the source
image's pixel coordinates (Resize's inverse label map, rounded to the nearest
pixel), and the overlay is drawn on the resampled frame.

With config.PEAKS set (a dict of KeypointsGauss.predict_peaks's keyword arguments)
the same forward's low-res logits also go through the multi-peak decode
(ops.heat_peaks): rank 0 saves preds/peaks.npy (float32 [n_images, K, max_peaks, 3]:
(x, y, score) per local maximum, sub-pixel, best first, unused slots (-1, -1, 0); with
RESIZE in each source image's pixels, unrounded) and preds/peak_counts.npy (int32
[n_images, K]), file order, all-gathered like the keypoints.  keypoints.npy and the
overlays are what they are without it.

With config.EVAL set and a label directory given (main's label_dir, or a third
command-line argument) the decoded peaks (EVAL's max_peaks / radius / threshold) are
also matched on the GPU to each image's labels and accumulated
(hkp.metrics.KeypointMetrics): labels are paired with the images by name as
KeypointsDataset pairs them (<image stem>.npy) and read as KeypointsDataset(instances=...)
reads them ([K,2], [K,3] or [K,m,3] (u, v, flag)).  Each rank accumulates its own
shard, the integer accumulators are summed once over the ranks (all_reduce), and rank 0
writes preds/metrics.json: KeypointMetrics.compute()'s dict (nan as null).  With
RESIZE set the peaks are mapped to each source image's pixels before the matching and
the labels are in source pixels, so EVAL's thresholds are distances in SOURCE pixels.
Everything else written is what it is without EVAL.

PEAKS and EVAL may each hold "tta": a dict of hkp.tta.TestTimeAugmentation's keyword
arguments.  The forward above is then view 0, every other view one more forward of the
same image, and that decode reads the merged logits (ops.logits_merge) instead of the
one forward's; keypoints.npy and the overlays still come from the plain forward.

PEAKS may also hold "groups": {"classes": (class indices), "max_dist": 1.0} (a model trained
with config.TAGS; not with "tta": tags are not merged across views).  The one forward then
runs the head over the fc rows 0..2K-1 — the heat channels, and with them everything above,
are the same bits — and rank 0 also saves preds/peak_groups.npy, int32 [n_images, K,
max_peaks]: the cable of every peak of peaks.npy, grouped by tag on the GPU
(ops.peaks_group, what KeypointsGauss.predict_groups returns), -1 for unused slots and
classes not listed.
"""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

from config import BACKBONE, EVAL, IMG_HEIGHT, IMG_WIDTH, NUM_KEYPOINTS, PEAKS, RESIZE, RESIZE_PARAMS
from hkp import net, ops, parallel
from src.dataset import imread_bgr, transform
from src.model import KeypointsGauss
from src.prediction import Prediction


def _json_safe(v):
    if isinstance(v, dict):
        return {k: _json_safe(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_json_safe(x) for x in v]
    return None if isinstance(v, float) and v != v else v


def main(model_ckpt="", image_dir="", out_dir="preds", checkpoint_dir="checkpoints", label_dir=None):
    world = int(os.environ.get("WORLD_SIZE", "1"))
    own_group = world > 1 and not dist.is_initialized()
    if world > 1:
        local = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(local)
        if own_group:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    keypoints = KeypointsGauss(NUM_KEYPOINTS, img_height=IMG_HEIGHT, img_width=IMG_WIDTH, backbone=BACKBONE,
                               pretrained=False)
    keypoints.load_state_dict(torch.load(os.path.join(checkpoint_dir, model_ckpt), map_location="cpu",
                                         weights_only=True))
    use_cuda = torch.cuda.is_available()
    if use_cuda:
        if world == 1:
            torch.cuda.set_device(0)
        keypoints = keypoints.cuda()
    prediction = Prediction(keypoints, NUM_KEYPOINTS, IMG_HEIGHT, IMG_WIDTH, use_cuda)
    files = sorted(os.listdir(image_dir))
    lo, hi = parallel.shard_range(len(files), parallel.rank(), parallel.world())
    kps, pks, cts = [], [], []
    npk = int(PEAKS.get("max_peaks", 4)) if PEAKS is not None else 0
    from hkp.tta import split_config
    peaks_kw, peaks_tta = split_config(PEAKS)
    groups_kw = peaks_kw.pop("groups", None) if peaks_kw is not None else None
    grs = []
    if groups_kw is not None:
        if peaks_tta is not None:
            raise ValueError("config.PEAKS: 'groups' does not go with 'tta' (tags are not merged across views)")
        if set(groups_kw) - {"classes", "max_dist"} or "classes" not in groups_kw:
            raise ValueError("config.PEAKS['groups'] holds classes and optionally max_dist, got %r" % (groups_kw,))
    metrics = eval_kw = eval_tta = None
    if EVAL is not None and label_dir:
        from hkp.metrics import from_config, load_labels
        metrics, eval_kw = from_config(EVAL, NUM_KEYPOINTS, device="cuda")
        eval_tta = eval_kw.pop("tta", None)

    def merged(tta, x, low):                         # the views' forwards beside the plain one (view 0)
        if tta is None:
            return low
        return tta.run(x, lambda xv: net.keypoints_forward(keypoints.resnet.net, xv, NUM_KEYPOINTS, heat=False,
                                                           argmax=False, pol=keypoints.policy, upsample=False)[2],
                       low0=low)
    for i in range(lo, hi):
        img = imread_bgr(os.path.join(image_dir, files[i]))
        print(img.shape)
        plan = None
        if RESIZE is not None and img.shape[:2] != (IMG_HEIGHT, IMG_WIDTH):
            from hkp.resample import Resize
            plan = Resize(filter=RESIZE, **RESIZE_PARAMS).plan([img.shape[:2]], (IMG_HEIGHT, IMG_WIDTH))
            flat = torch.from_numpy(np.ascontiguousarray(img).reshape(-1)).cuda()
            img = ops.resample_ragged_u8(flat, plan)[0].cpu().numpy()
        img_t = transform(img).cuda()
        with torch.no_grad():
            if PEAKS is None and metrics is None:
                heatmap, kp = keypoints.heatmaps_and_keypoints(img_t.view(-1, *img_t.shape))
            else:                                    # the same forward; its low-res logits feed the peak decode
                heatmap, kp, low = net.keypoints_forward(keypoints.resnet.net, img_t.view(-1, *img_t.shape),
                                                         NUM_KEYPOINTS, heat=True, argmax=True, pol=keypoints.policy,
                                                         tags=groups_kw is not None)
                if groups_kw is not None:            # low_all: heat logits, then the tag maps
                    low_all, low = low, low[:, :NUM_KEYPOINTS].contiguous()
            if PEAKS is not None:
                pk, ct = ops.heat_peaks(merged(peaks_tta, img_t.view(-1, *img_t.shape), low), IMG_HEIGHT, IMG_WIDTH,
                                        **peaks_kw)
                if groups_kw is not None:            # grouped on the network's own frame
                    grs.append(ops.peaks_group(pk, ct, low_all, IMG_HEIGHT, IMG_WIDTH, groups_kw["classes"],
                                               max_dist=groups_kw.get("max_dist", 1.0))[0][0])
                if plan is not None:                 # (x, y) of the used slots -> the source image's pixels
                    pk = plan.invert_peaks(pk.cpu(), ct.cpu()).to(pk.device)
                pks.append(pk[0])
                cts.append(ct[0])
            if metrics is not None:                  # EVAL's own decode, matched to this image's labels
                pk, ct = ops.heat_peaks(merged(eval_tta, img_t.view(-1, *img_t.shape), low), IMG_HEIGHT, IMG_WIDTH,
                                        **eval_kw)
                if plan is not None:
                    pk = plan.invert_peaks(pk.cpu(), ct.cpu()).to(pk.device)
                lab = load_labels(os.path.join(label_dir, os.path.splitext(files[i])[0] + ".npy"), NUM_KEYPOINTS)
                metrics.update(pk, ct, torch.from_numpy(lab[None]).to(pk.device))
        prediction.plot(img, heatmap.cpu().numpy(), image_id=i, keypoints=kp.cpu().numpy(), out_dir=out_dir)
        if plan is not None:                         # (y, x) on the resampled frame -> the source image's pixels
            uv = plan.invert_uv(kp[:1].cpu().numpy()[..., ::-1].astype(np.float32))
            kp = torch.from_numpy(np.rint(uv[..., ::-1]).astype(np.int32)).to(kp.device)
        kps.append(kp[0])
    local_kp = torch.stack(kps) if kps else torch.zeros((0, NUM_KEYPOINTS, 2), dtype=torch.int32, device="cuda")
    all_kp = parallel.gather_keypoints(local_kp).cpu().numpy()
    if PEAKS is not None:
        local_pk = torch.stack(pks) if pks else torch.zeros((0, NUM_KEYPOINTS, npk, 3), dtype=torch.float32,
                                                            device="cuda")
        local_ct = torch.stack(cts) if cts else torch.zeros((0, NUM_KEYPOINTS), dtype=torch.int32, device="cuda")
        all_pk, all_ct = (t.cpu().numpy() for t in parallel.gather_peaks(local_pk, local_ct))
        if groups_kw is not None:
            local_gr = torch.stack(grs) if grs else torch.zeros((0, NUM_KEYPOINTS, npk), dtype=torch.int32,
                                                                device="cuda")
            all_gr = parallel.gather_groups(local_gr).cpu().numpy()
    if metrics is not None:
        metrics.all_reduce()
    if parallel.rank() == 0:
        os.makedirs(out_dir, exist_ok=True)
        np.save(os.path.join(out_dir, "keypoints.npy"), all_kp)
        if metrics is not None:
            import json
            with open(os.path.join(out_dir, "metrics.json"), "w") as f:
                json.dump(_json_safe(metrics.compute()), f, indent=1)
        if PEAKS is not None:
            np.save(os.path.join(out_dir, "peaks.npy"), all_pk)
            np.save(os.path.join(out_dir, "peak_counts.npy"), all_ct)
            if groups_kw is not None:
                np.save(os.path.join(out_dir, "peak_groups.npy"), all_gr)
    if own_group:
        dist.destroy_process_group()
    return all_kp


if __name__ == "__main__":
    main(*sys.argv[1:3], label_dir=sys.argv[3] if len(sys.argv) > 3 else None)
