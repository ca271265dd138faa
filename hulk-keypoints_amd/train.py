"""train.py of the reference (train.py:1-82) on the MI355X path.

Same ``forward(sample_batched, model)`` and ``fit(train_data, test_data, model,
epochs, checkpoint_path='')`` surface, same prints and checkpoint names
(model_2_1_<epoch>.pth every 2 epochs, reference state_dict keys).  The loss
is the fused HIP BCE kernel (bit-for-bit the math of nn.BCELoss on
pred.double(), train.py:21,25).

Data parallel: launch with ``torchrun --nproc-per-node N train.py``; each rank
takes a DistributedSampler shard, gradients are all-reduced over RCCL in
buckets overlapped with the backward kernels: the model's grad_ready hook hands
each gradient to hkp.train.GradBucketer as the backward produces it inside
loss.backward(), a full bucket's all-reduce starts right away, and
_reduce_grads only waits for the last ones.  Rank 0 prints and checkpoints.

With config.EVAL set (default None: nothing changes) the test loop makes one forward
per batch under no_grad, takes the test loss from its heatmaps and the decoded peaks
from its low-res logits, matches them to the labels on the GPU
(hkp.metrics.KeypointMetrics) and prints one more line, `test eval: ...`, after
`test loss:`.  Every rank walks the whole test set, so no reduction is needed.

With config.MAX_GRAD_NORM or config.EMA_DECAY set (default None: nothing changes) main()
builds hkp.optim.FusedAdam with those options instead of torch's Adam: the gradients are
clipped by their global L2 norm (after the all-reduce under data parallelism) and / or
an exponential moving average of the parameters is kept.  With an EMA the test loop
runs on the averaged weights (optimizer.ema_weights()), and next to each
model_2_1_<epoch>.pth (the raw weights, needed to resume) fit() writes
model_2_1_<epoch>_ema.pth.  The EMA covers the parameters; BN running statistics are
buffers and are saved as they stand.

With config.SYNTH set (default None: nothing changes) main() needs no data/ directory: both
sets are procedural cable scenes rendered on the GPU (hkp.synth.CableScenes through
src.dataset.SynthDataset) with instance labels [K,M,3]; the train set draws new scenes every
epoch, the test set is fixed and comes from seed + 1.  NUM_KEYPOINTS must equal the number
of classes; GEOMETRIC_AUGMENTATION and RESIZE do not go with it here (DeviceBatches takes
geometric= for a SynthDataset).  When config.SYNTH["classes"] holds a line class
(hkp.synth.LINE_CLASSES: "cable", labelled by its centreline's pieces), both sets are built with
return_uv=False: the items carry the dense target of hkp_line_target over points and segments
together, the reference's dense target -> BCE path, which _loss takes as it stands.  EVAL and
TAGS need point labels and raise at start-up with such scenes.

With config.LOSS = "qfl" (default "bce": nothing changes) the train and the test loop take
the quality focal loss of hkp_heat_loss_multi_ex, with config.LOSS_PARAMS's beta and norm;
it needs point labels ((u, v) or instances), which main()'s datasets give.

config.LOSS_PARAMS may also hold "class_weights" (K floats: a weight per keypoint class, put on
the device once) and "topk" (per image only that many classes with the largest weighted loss
are trained: hard keypoint mining), both through hkp_heat_loss_planes and point labels only.
With config.CLASS_LOSS = True (default False: nothing changes) the loss also returns its
value per (image, class) plane; fit() adds them up per class on the device, over the planes
that took part in the labels (plane_loss >= 0), reads the sums once per epoch and prints
`train class loss: c0 ... cK-1` after `train loss:` and `test class loss: ...` after
`test loss:`: the unweighted mean loss per pixel of each class (nan for a class that no
image labelled).  Under data parallelism rank 0 prints its own shard's train values.
With config.TAGS set (default None: nothing changes) — {"classes": ("cap", "tail"), "weight":
1e-3, "pull": 1.0, "push": 1.0}, classes as indices or as names of config.SYNTH["classes"] —
the train loop steps an hkp.train.Trainer built with tags=: the head also computes one tag map
per class (fc rows K..2K-1), the pull / push loss of hkp_tag_loss trains the tags of one cable
together and those of different cables apart (slot m of every listed class is cable m), and
fit() prints `train tag loss: total pull push` after `train loss:`, summed on the GPU and read
once per epoch.  The labels must be instances [B,K,M,3] (INSTANCES or SYNTH); the optimizer is
the Trainer's FusedAdam (lr 1e-4, weight decay 1e-4, with MAX_GRAD_NORM / EMA_DECAY); the test
loop is unchanged.  TAGS does not go with CLASS_LOSS.
"""
import contextlib
import os
import sys

import torch
import torch.distributed as dist
from torch.utils.data import DataLoader

from config import *  # noqa: F401,F403
from config import (ABSENT, BACKBONE, CLASS_LOSS, DOMAIN_RANDOMIZATION, DR_SEED, EMA_DECAY, EVAL, GA_PARAMS, GA_SEED,
                    GAUSS_SIGMA, GEOMETRIC_AUGMENTATION, IMG_HEIGHT, IMG_WIDTH, INSTANCES, LOSS, LOSS_PARAMS,
                    MAX_GRAD_NORM, NUM_KEYPOINTS, RESIZE, RESIZE_PARAMS, SYNTH, TAGS, batch_size, epochs)
from hkp import autograd as hkp_autograd
from hkp import net, ops
from hkp.train import GradBucketer, broadcast_state
from src.dataset import KeypointsDataset, SynthDataset, domain_randomization, transform
from src.model import KeypointsGauss

use_cuda = True
optimizer = None
keypoints = None
_bucketer = None
_class_weights = {}     # device -> LOSS_PARAMS["class_weights"] as a float32 tensor, built once
_class_acc = None       # CLASS_LOSS: float64 [2,K] on the device, per class the sum of plane_loss and the planes
_trainer = None         # TAGS: the hkp.train.Trainer that steps the train loop


def _rank0():
    return not dist.is_initialized() or dist.get_rank() == 0


def forward(sample_batched, model):
    img, gt = sample_batched
    img = img.cuda(non_blocking=True)
    return _loss(model.forward(img), gt)


def _planes_kw(pred_gauss):
    """LOSS_PARAMS' class_weights as heatmap_loss's weights [B,K] (the other keys pass as they
    are), and return_planes with CLASS_LOSS; the parameters unchanged when neither is set."""
    if "class_weights" not in LOSS_PARAMS and "lines" not in LOSS_PARAMS and not CLASS_LOSS:
        return LOSS_PARAMS
    # "lines" is hkp.train.Trainer's route for line labels; these loops read point labels
    kw = {k: v for k, v in LOSS_PARAMS.items() if k not in ("class_weights", "lines")}
    if "class_weights" in LOSS_PARAMS:
        dev = pred_gauss.device
        key = (dev, tuple(float(v) for v in LOSS_PARAMS["class_weights"]))
        if key not in _class_weights:
            _class_weights[key] = torch.tensor(key[1], dtype=torch.float32, device=dev)
        if _class_weights[key].numel() != pred_gauss.shape[1]:
            raise ops.HkpError("LOSS_PARAMS['class_weights'] must hold %d floats" % pred_gauss.shape[1])
        kw["weights"] = _class_weights[key][None, :].expand(pred_gauss.shape[0], -1).contiguous()
    if CLASS_LOSS:
        kw["return_planes"] = True
    return kw


def _class_loss_add(out):
    """heatmap_loss(return_planes=True)'s result: the per-class sums go into _class_acc on
    the device (no synchronisation); returns the loss."""
    global _class_acc
    loss, plane_loss, _ = out
    on = plane_loss >= 0
    add = torch.stack([torch.where(on, plane_loss, torch.zeros_like(plane_loss)).sum(0), on.sum(0).double()])
    _class_acc = add if _class_acc is None else _class_acc + add
    return loss


def _class_loss_line(what):
    """Prints `<what> class loss: c0 ... cK-1` from _class_acc (its one read) and clears it."""
    global _class_acc
    if _class_acc is not None and _rank0():
        sums, cnt = _class_acc.tolist()
        print(what + " class loss:", *[s / c if c else float("nan") for s, c in zip(sums, cnt)])
    _class_acc = None


def _loss(pred_gauss, gt):
    kw = _planes_kw(pred_gauss)
    done = _class_loss_add if CLASS_LOSS else (lambda out: out)
    if gt.dim() == 3:   # (u, v) labels → the loss kernel recomputes the Gaussian target in registers
        return done(hkp_autograd.heatmap_loss(pred_gauss, uv=gt.cuda().float().contiguous(), sigma=GAUSS_SIGMA,
                                              kind=LOSS, **kw))
    if gt.dim() == 4 and gt.shape != pred_gauss.shape and gt.shape[-1] == 3 and gt.is_floating_point():
        # instance labels [B,K,M,3] (u, v, flag): the multi-instance target, absent planes per ABSENT
        return done(hkp_autograd.heatmap_loss(pred_gauss, pts=gt.cuda().float().contiguous(), sigma=GAUSS_SIGMA,
                                              kind=LOSS, absent=ABSENT, **kw))
    return done(hkp_autograd.heatmap_loss(pred_gauss, target=gt.cuda().double().contiguous(), kind=LOSS, **kw))


def eval_forward(sample_batched, model, metrics, peak_kw):
    """The test step with config.EVAL set: ONE forward under no_grad gives the test
    loss (from its heatmaps) and, from its low-res logits, the decoded peaks, which one
    more launch matches to the batch's labels and adds into `metrics`
    (hkp.metrics.KeypointMetrics); no host synchronisation beyond the caller's
    loss.item().  The labels must be (u, v) [B,K,2] or instances [B,K,M,3].
    With EVAL's "tta" (peak_kw["tta"], a hkp.tta.TestTimeAugmentation) that forward
    still gives the test loss and is view 0; the other views are extra forwards under
    the same no_grad, and the peaks are those of the merged logits."""
    img, gt = sample_batched
    peak_kw = dict(peak_kw)
    tta = peak_kw.pop("tta", None)
    dense = (img.shape[0], model.num_keypoints) + tuple(net.image_nchw_shape(img)[2:])
    if tuple(gt.shape) == dense or not (gt.dim() == 3 or (gt.dim() == 4 and gt.shape[-1] == 3)):
        raise ops.HkpError("EVAL needs point labels ([B,K,2] or [B,K,M,3]), not dense targets %s: build the test "
                           "set with return_uv=True" % (tuple(gt.shape),))
    img = img.cuda(non_blocking=True)
    with torch.no_grad():
        heat, _, low = net.keypoints_forward(model.resnet.net, img, model.num_keypoints, heat=True, argmax=False,
                                             pol=model.policy)
        loss = _loss(heat, gt)
        H, W = net.image_nchw_shape(img)[2:]
        if tta is not None:
            low = tta.run(img, lambda xv: net.keypoints_forward(model.resnet.net, xv, model.num_keypoints, heat=False,
                                                                argmax=False, pol=model.policy, upsample=False)[2],
                          low0=low)
        peaks, counts = ops.heat_peaks(low, H, W, **peak_kw)
        metrics.update(peaks, counts, gt.cuda().float().contiguous())
    return loss


def _reduce_grads(model):
    """After loss.backward(): wait for the bucket all-reduces the backward already
    launched (model.grad_ready = GradBucketer.ready) and point p.grad at the
    averaged buckets."""
    if _bucketer is None:
        return
    _bucketer.finish()


def setup_data_parallel(model, bucket_mb=32):
    """DP wiring (torchrun): every rank starts from rank 0's parameters and BN
    buffers, and the backward hands each gradient to the bucketer as soon as it
    exists (model.grad_ready), so bucket all-reduces overlap the backward."""
    global _bucketer
    broadcast_state(model)
    _bucketer = GradBucketer(list(model.parameters()), bucket_mb << 20)
    model.grad_ready = _bucketer.ready
    return _bucketer


def _ema_weights():
    """optimizer.ema_weights() if the optimizer keeps an EMA (hkp.optim.FusedAdam with
    ema_decay), else a context that does nothing."""
    if hasattr(optimizer, "ema_weights") and any(g.get("ema_decay") is not None for g in optimizer.param_groups):
        return optimizer.ema_weights(), True
    return contextlib.nullcontext(), False


def _tags_config():
    """config.TAGS as Trainer's tags= : class names go through config.SYNTH["classes"]."""
    tags = dict(TAGS)
    names = tuple(SYNTH["classes"]) if SYNTH is not None and "classes" in SYNTH else ()
    classes = []
    for c in tags.get("classes", ()):
        if isinstance(c, str):
            if c not in names:
                raise ValueError("config.TAGS: class %r is not in config.SYNTH['classes'] %r" % (c, names))
            c = names.index(c)
        classes.append(c)
    tags["classes"] = tuple(classes)
    return tags


def _tags_trainer(model):
    """The Trainer of the train loop under config.TAGS (built once per model); its optimizer
    becomes this module's."""
    global _trainer, optimizer
    if _trainer is None or _trainer.model is not model:
        from hkp.train import Trainer
        if CLASS_LOSS:
            raise ValueError("config.TAGS does not go with CLASS_LOSS")
        _trainer = Trainer(model, lr=1.0e-4, weight_decay=1.0e-4, loss=LOSS, sigma=GAUSS_SIGMA, absent=ABSENT,
                           distributed=dist.is_initialized(), max_grad_norm=MAX_GRAD_NORM, ema_decay=EMA_DECAY,
                           loss_params=LOSS_PARAMS, tags=_tags_config())
        optimizer = _trainer.opt
    return _trainer


def _tags_step(trainer, sample_batched):
    img, gt = sample_batched
    if not (gt.dim() == 4 and gt.shape[-1] == 3 and gt.is_floating_point()):
        raise ops.HkpError("config.TAGS needs instance labels [B,K,M,3] (INSTANCES or SYNTH), got %s"
                           % (tuple(gt.shape),))
    return trainer.step(img.cuda(non_blocking=True), pts=gt.cuda().float().contiguous())


def fit(train_data, test_data, model, epochs, checkpoint_path=""):
    metrics = peak_kw = None
    trainer = _tags_trainer(model) if TAGS is not None else None
    if EVAL is not None:            # every rank walks the whole test set: no reduction needed
        from hkp.metrics import from_config
        metrics, peak_kw = from_config(EVAL, model.num_keypoints)
    global _class_acc
    for epoch in range(epochs):
        _class_acc = None
        if hasattr(getattr(train_data, "sampler", None), "set_epoch"):
            train_data.sampler.set_epoch(epoch)
        if hasattr(getattr(train_data, "dataset", None), "set_epoch"):
            train_data.dataset.set_epoch(epoch)     # the geometric augmentation draws per (seed, epoch, index)
        train_loss = 0.0
        i_batch = 0
        tag_acc, tag_steps = None, 0
        for i_batch, sample_batched in enumerate(train_data):
            if trainer is not None:
                loss = _tags_step(trainer, sample_batched)
                tag_acc = trainer.tag_loss if tag_acc is None else tag_acc + trainer.tag_loss
                tag_steps += 1
            else:
                optimizer.zero_grad()
                loss = forward(sample_batched, model)
                loss.backward()
                _reduce_grads(model)
                optimizer.step()
            train_loss += loss.item()
            if _rank0():
                print("[%d, %5d] loss: %.3f" % (epoch + 1, i_batch + 1, loss.item()), end="")
                print("\r", end="")
        if _rank0():
            print("train loss:", train_loss / max(i_batch, 1))   # reference divides by i_batch (train.py:40)
            if tag_acc is not None:
                print("train tag loss:", *[v / tag_steps for v in tag_acc.tolist()])
        _class_loss_line("train")
        test_loss = 0.0
        i_batch = 0
        if metrics is not None:
            metrics.reset()
        ema_ctx, has_ema = _ema_weights()
        with ema_ctx:                   # with an EMA: the test loop and the _ema checkpoint on the averaged weights
            for i_batch, sample_batched in enumerate(test_data):
                if metrics is None:
                    loss = forward(sample_batched, model)
                else:
                    loss = eval_forward(sample_batched, model, metrics, peak_kw)
                test_loss += loss.item()
            if _rank0():
                print("test loss:", test_loss / max(i_batch, 1))
            _class_loss_line("test")
            if _rank0():
                if metrics is not None:
                    print("test eval:", metrics.summary())
                if has_ema and epoch % 2 == 0:
                    torch.save(model.state_dict(), checkpoint_path + "/model_2_1_" + str(epoch) + "_ema.pth")
        if _rank0():
            if epoch % 2 == 0:
                torch.save(model.state_dict(), checkpoint_path + "/model_2_1_" + str(epoch) + ".pth")


def main(dataset_dir="", output_dir="checkpoints", workers=0):
    global optimizer, keypoints
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        local = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    else:
        torch.cuda.set_device(0)
    save_dir = os.path.join(output_dir, dataset_dir)
    if _rank0():
        os.makedirs(save_dir, exist_ok=True)
    # the reference switches its augmentation on by moving a '#' (dataset.py:15-31); here it is a config
    # key, and only the train set is randomised.  The transform runs on the GPU: keep workers at 0.
    train_transform = domain_randomization(seed=DR_SEED) if DOMAIN_RANDOMIZATION else transform
    geometric = None
    if GEOMETRIC_AUGMENTATION:                      # images and labels together; the train set only
        from hkp.geometry import GeometricAugmentation
        geometric = GeometricAugmentation(seed=GA_SEED, **GA_PARAMS)
    resize = None
    if RESIZE is not None:                          # image files of any size; train and test set alike
        from hkp.resample import Resize
        resize = Resize(filter=RESIZE, **RESIZE_PARAMS)
    if SYNTH is not None:                           # procedural scenes: no data/ directory
        from hkp.synth import from_config as synth_from_config
        if geometric is not None or resize is not None:
            raise ValueError("config.SYNTH does not go with GEOMETRIC_AUGMENTATION or RESIZE in train.py")
        train_scenes, test_scenes, n_train, n_test = synth_from_config(SYNTH, NUM_KEYPOINTS)
        dense = {}
        if train_scenes.line_slots:                 # a line class: the items carry the dense target
            if EVAL is not None or TAGS is not None:
                raise ValueError("config.SYNTH['classes'] %r holds a line class: its items are dense targets, and "
                                 "config.EVAL and config.TAGS need point labels" % (train_scenes.classes,))
            dense = {"return_uv": False}
        train_dataset = SynthDataset(train_scenes, n_train, (IMG_HEIGHT, IMG_WIDTH), transform=train_transform,
                                     gauss_sigma=GAUSS_SIGMA, **dense)
        test_dataset = SynthDataset(test_scenes, n_test, (IMG_HEIGHT, IMG_WIDTH), fixed=True, gauss_sigma=GAUSS_SIGMA,
                                    **dense)
    else:
        train_dataset = KeypointsDataset("data/%s/train/images" % dataset_dir,
                                         "data/%s/train/keypoints" % dataset_dir, NUM_KEYPOINTS, IMG_HEIGHT,
                                         IMG_WIDTH, train_transform, gauss_sigma=GAUSS_SIGMA, return_uv=True,
                                         geometric=geometric, resize=resize, instances=INSTANCES)
        test_dataset = KeypointsDataset("data/%s/test/images" % dataset_dir, "data/%s/test/keypoints" % dataset_dir,
                                        NUM_KEYPOINTS, IMG_HEIGHT, IMG_WIDTH, transform, gauss_sigma=GAUSS_SIGMA,
                                        return_uv=True, resize=resize, instances=INSTANCES)
    sampler = torch.utils.data.distributed.DistributedSampler(train_dataset) if world > 1 else None
    train_data = DataLoader(train_dataset, batch_size=batch_size, shuffle=sampler is None, sampler=sampler,
                            num_workers=workers)
    test_data = DataLoader(test_dataset, batch_size=batch_size, shuffle=True, num_workers=workers)
    keypoints = KeypointsGauss(NUM_KEYPOINTS, img_height=IMG_HEIGHT, img_width=IMG_WIDTH, backbone=BACKBONE).cuda()
    if TAGS is not None:                # the Trainer steps the train loop with its own FusedAdam
        _tags_trainer(keypoints)
    elif MAX_GRAD_NORM is None and EMA_DECAY is None:
        optimizer = torch.optim.Adam(keypoints.parameters(), lr=1.0e-4, weight_decay=1.0e-4)   # train.py:79
    else:                               # the same step with clipping and / or a weight EMA in its one pass
        from hkp.optim import FusedAdam
        optimizer = FusedAdam(keypoints.parameters(), lr=1.0e-4, weight_decay=1.0e-4, max_grad_norm=MAX_GRAD_NORM,
                              ema_decay=EMA_DECAY)
    if world > 1 and TAGS is None:
        setup_data_parallel(keypoints)
    fit(train_data, test_data, keypoints, epochs=epochs, checkpoint_path=save_dir)
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main(*sys.argv[1:2])
