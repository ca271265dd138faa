"""config.py of the reference (config.py:1-6), same names and defaults.

Additive keys (defaults reproduce the reference): BACKBONE, LOSS
('bce' is what train.py:25 uses; 'mse' is train.py:13's unused MSE; 'qfl' is the quality
focal loss, not in the reference: BCE against the Gaussian target scaled per pixel by
|target - heat|^beta, so the many easy background pixels stop dominating the sum while
the minimum stays at heat == target, hkp_heat_loss_multi_ex; point labels only) and
LOSS_PARAMS (the other keyword arguments of that loss: {} for 'bce' and 'mse'; for 'qfl'
beta in [1, 8], default 2.0, and norm, "elements": the mean over the pixels, the default,
or "instances": the sum over the pixels divided by the number of keypoint instances
present in the batch, at least 1; "instances" also goes with 'bce' / 'mse' when INSTANCES
is set),
DOMAIN_RANDOMIZATION (True: the train set goes through the reference's commented-out
augmentation pipeline, dataset.py:18-31, on the GPU) and DR_SEED (its seed),
GEOMETRIC_AUGMENTATION (True: the train set's images and labels go through
hkp.geometry.GeometricAugmentation — rotation, scale, translation, flips; not in the
reference), GA_SEED (its seed) and GA_PARAMS (its other keyword arguments),
RESIZE (None: every image file already has IMG_WIDTH x IMG_HEIGHT, as the reference
assumes; a filter name — "box", "bilinear", "hamming", "bicubic", "lanczos" — : files
of any size are resampled on the GPU to that size, antialiased, hkp.resample.Resize,
with the labels in each file's own pixel coordinates) and RESIZE_PARAMS (its other
keyword arguments: mode="stretch" / "fit", fill=(B, G, R)), PEAKS (None: analysis.py
writes what the reference writes; a dict of KeypointsGauss.predict_peaks's keyword
arguments, e.g. {"max_peaks": 4, "radius": 1, "threshold": 0.1}: analysis.py also
writes preds/peaks.npy — float32 [n_images, K, max_peaks, 3], (x, y, score) per local
maximum of each heatmap, sub-pixel, best first, unused slots (-1, -1, 0), in each
source image's pixels when RESIZE is set — and preds/peak_counts.npy, int32
[n_images, K]; keypoints.npy and the overlays do not change), INSTANCES (None: one
(u, v) per keypoint, clipped onto the image, as the reference; M in 1..16: the label
files may hold [K,2], [K,3] or [K,m,3] (u, v, flag) with m <= M, a keypoint class may
have several instances or none, points outside the image are marked absent instead
of clipped, and the loss runs against the maximum of the instances' Gaussians,
hkp_heat_loss_multi) and ABSENT ("zero": a keypoint that is not in the picture is
trained against the all-zero heatmap; "ignore": its plane is left out of the loss),
EVAL (None: train.py and analysis.py report what the reference reports; a dict such as
{"thresholds": (2, 4, 8, 16), "max_peaks": 4, "radius": 1, "threshold": 0.1} — also
"bins" —: the test loop of train.py's fit() decodes the peaks of its one forward per
batch, matches them to the labels on the GPU (hkp.metrics.KeypointMetrics) and prints
one more line after `test loss:` with the recall per distance threshold (pixels), the
mAP and the mean localisation error; analysis.py, given a label directory, writes
preds/metrics.json), MAX_GRAD_NORM (None: the reference's bare Adam step; a float > 0:
train.py's optimizer is hkp.optim.FusedAdam and clips the gradients by their global L2
norm to that value before each step, on the GPU) and EMA_DECAY (None; a float strictly
between 0.5 and 1: FusedAdam also keeps an exponential moving average of the parameters,
fit() runs its test loop on it and writes model_2_1_<epoch>_ema.pth next to each
checkpoint), and, through hkp_heat_loss_planes and with point labels only: LOSS_PARAMS may
also hold "class_weights" (K floats, a weight per keypoint class: its planes' loss and gradient
are scaled by it, a weight of 0 takes the class out of the loss) and "topk" (an int in 1..K:
hard keypoint mining, per image only that many classes with the largest weighted loss are
trained), and "lines" ("dense", the default: a Trainer step with line labels writes the dense
target and runs the dense loss; "walk": it makes one hkp_heat_loss_lines call, the target in
registers, and every loss choice of the point labels holds for line planes too; train.py's own
loops read no line labels and pass the key over), and CLASS_LOSS (False; True: fit() prints `train class loss:` and `test class
loss:` lines with the mean loss per pixel of each class, summed on the GPU and read once per
epoch), and SYNTH (None: train.py reads data/<dataset>/ as the reference does; a dict such as
{"train": 512, "test": 128, "seed": 0, "classes": ("cap", "tail", "crossing", "blob"),
"instances": 8} — "train" and "test" are scenes per epoch, every other key a keyword argument of
hkp.synth.CableScenes —: train.py's main() needs no data/ directory, both sets are procedural
cable scenes rendered on the GPU, hkp_synth_cables_u8, with instance labels [K,M,3] of M =
"instances" slots; the train set draws new scenes every epoch, the test set is fixed and
comes from seed + 1; NUM_KEYPOINTS must equal the number of classes).
PEAKS and EVAL each also take "tta": a dict of hkp.tta.TestTimeAugmentation's keyword
arguments, e.g. {"hflip": True, "flip_pairs": ((0, 1),), "mode": "prob"} — test-time
augmentation: the decode then reads the logits of several views (mirrored, rescaled), one
forward each, merged on the stride-8 lattice by one launch, hkp_logits_merge.  The plain
forward is view 0 and still gives `test loss:`, keypoints.npy and the overlays; the other
views are extra forwards under the same no_grad (in train-mode BN each takes its own batch
statistics and moves the running ones).  Scaled views ("scales") need uint8 NHWC batches:
analysis.py and a test set of fp32 tensors take flips only.  An unknown key raises.
TAGS (None: nothing changes; a dict such as {"classes": ("cap", "tail"), "weight": 1e-3, "pull":
1.0, "push": 1.0} — classes as indices or as names of SYNTH["classes"] —: associative-embedding
tags, which keypoints belong to one cable.  train.py's train loop steps hkp.train.Trainer(tags=):
fc row K + c becomes the tag map of class c (2 * NUM_KEYPOINTS <= 16), trained by hkp_tag_loss
with instance labels whose slot m is cable m, and fit() prints one more line, `train tag loss:
total pull push`, after `train loss:`).  PEAKS also takes "groups": {"classes": (class indices),
"max_dist": 1.0}: analysis.py then also writes preds/peak_groups.npy, int32 [n_images, K,
max_peaks], the cable of every peak of peaks.npy (KeypointsGauss.predict_groups; -1: none); it
does not go with "tta".
"""
NUM_KEYPOINTS = 4
IMG_HEIGHT = 480
IMG_WIDTH = 640
GAUSS_SIGMA = 8
epochs = 25
batch_size = 4

BACKBONE = "resnet34"
LOSS = "bce"
LOSS_PARAMS = {}
DOMAIN_RANDOMIZATION = False
DR_SEED = 0
GEOMETRIC_AUGMENTATION = False
GA_SEED = 0
GA_PARAMS = {}
RESIZE = None
RESIZE_PARAMS = {}
PEAKS = None
INSTANCES = None
ABSENT = "zero"
EVAL = None
MAX_GRAD_NORM = None
EMA_DECAY = None
CLASS_LOSS = False
SYNTH = None
TAGS = None
