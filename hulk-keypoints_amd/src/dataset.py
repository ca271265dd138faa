"""MI355X-native restatement of src/dataset.py's call surface.

  transform         dataset.py:16   ToTensor: HWC uint8 (BGR, as cv2.imread gives) → CHW fp32 / 255
  gauss_2d_batch    dataset.py:36-44  the Gaussian target, computed by the HIP kernel
                    hkp_gauss_target (fp32 arithmetic, fp64 result, on the GPU like the
                    reference's .cuda() meshgrid)
  KeypointsDataset  dataset.py:52-79  same constructor, same (img, gaussians) items; with
                    return_uv=True items are (img, uv) so the fused loss kernel recomputes
                    the target in registers instead of reading a [K,H,W] fp64 tensor.
  DeviceBatches     SURVEY §8(f1): the device data path — images decoded by `workers`
                    DataLoader processes (the reference decodes one image at a time in
                    the training process, dataset.py:71 with num_workers=0,
                    train.py:51), batched as uint8 HWC in pinned host memory, copied
                    asynchronously (3 B/pixel instead of the 12 B/pixel fp32 tensor,
                    one batch ahead on a side stream) and fed to the model as
                    [B,H,W,3] uint8, where the stem's operand pack applies ToTensor;
                    labels travel as (u, v) and the loss kernel makes the target.
  SynthDataset      not in the reference: procedural cable scenes (hkp.synth.CableScenes)
                    rendered on the GPU, hkp_synth_cables_u8, with instance labels from the
                    scene description; DeviceBatches takes a branch of its own for it (no
                    workers, no host image, no copy).
"""
import os

import numpy as np
import torch
import torch.nn.functional as F
from torch.utils.data import Dataset

from hkp import ops


def _to_tensor(img):
    """torchvision ToTensor semantics for an HWC uint8 array."""
    a = np.asarray(img)
    if a.ndim == 2:
        a = a[:, :, None]
    t = torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))
    return t.to(torch.float32).div_(255.0) if a.dtype == np.uint8 else t.to(torch.float32)


class Compose:
    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, x):
        for t in self.transforms:
            x = t(x)
        return x


# No domain randomization (dataset.py:15-16)
transform = Compose([_to_tensor])


def domain_randomization(seed=0, random_order=True, ops=None):
    """The reference's commented-out transform (dataset.py:18-31): the eight imgaug
    colour / blur / noise augmenters in random order, then ToTensor — here
    hkp.augment.DomainRandomization (one HIP kernel, csrc/augment.hip) composed
    with ToTensor.  For the device data path pass the DomainRandomization object
    itself: DeviceBatches(..., augment=DomainRandomization(seed))."""
    from hkp.augment import DomainRandomization
    return Compose([DomainRandomization(seed=seed, random_order=random_order, ops=ops), _to_tensor])


def imread_bgr(path):
    """cv2.imread (BGR uint8 HWC) when OpenCV is installed, else PIL converted to BGR."""
    try:
        import cv2  # noqa: F401
        img = cv2.imread(path)
        if img is None:
            raise FileNotFoundError(path)
        return img
    except ImportError:
        from PIL import Image
        with Image.open(path) as im:
            return np.asarray(im.convert("RGB"))[:, :, ::-1].copy()


def normalize(x):
    return F.normalize(x, p=1)


def gauss_2d_batch(width, height, sigma, U, V, normalize_dist=False):
    """[K] U (column) and V (row) → [K, height, width] float64 Gaussians on the GPU.

    Same values as dataset.py:36-44 (exp in fp32, then .double()); unlike the
    reference it does not mutate U/V in place (dataset.py:37-38)."""
    dev = U.device if torch.is_tensor(U) and U.is_cuda else torch.device("cuda")
    u = torch.as_tensor(U).reshape(-1).to(dev, torch.float32)
    v = torch.as_tensor(V).reshape(-1).to(dev, torch.float32)
    uv = torch.stack([u, v], -1).reshape(1, -1, 2).contiguous()
    G = ops.gauss_target(uv, height, width, sigma)[0]
    if normalize_dist:
        return normalize(G.float()).double()
    return G


def vis_gauss(gaussians):
    """dataset.py:46-50: min-max normalised first Gaussian → test.png."""
    g = gaussians[0].detach().cpu().numpy()
    g = (g - g.min()) / max(g.max() - g.min(), 1e-12) * 255.0
    from PIL import Image
    Image.fromarray(g.astype(np.uint8)).save("test.png")


class KeypointsDataset(Dataset):
    def __init__(self, img_folder, labels_folder, num_keypoints, img_height, img_width, transform, gauss_sigma=8,
                 return_uv=False, device="cuda", geometric=None, resize=None, instances=None):
        """instances: None (the reference's labels: one (u, v) per keypoint, clipped onto the
        image), or M (1..16): multi-instance labels pts [K,M,3] (u, v, flag; flag > 0: the
        slot holds an instance).  A label file may then be [K,2] (every keypoint present
        once), [K,3] or [K,m,3] with m <= M; it is padded with empty slots.  Labels are
        not clipped: a present point outside the image is marked absent (flag 0) — with
        `resize`, after the resize has mapped it.  Items are (img, pts) with
        return_uv=True, else (img, gaussians) from hkp_gauss_target_multi; raw() returns
        pts.

        geometric: a hkp.geometry.GeometricAugmentation, or None.  When set, the decoded
        uint8 image and the host label go through it (on the GPU: keep num_workers=0)
        before `transform`, under the sample's own index and the epoch of set_epoch();
        the returned uv / Gaussians come from the transformed label.

        resize: a hkp.resample.Resize, or None.  When set, the image files may have any
        size: the stored labels stay in each file's own pixel coordinates (not clipped
        at load), and every decoded image is resampled on the GPU (antialiased,
        hkp_resample_u8; keep num_workers=0) to (img_height, img_width) before
        `geometric`, its label mapped by the same transform and then clipped."""
        self.geometric = geometric
        self.resize = resize
        self.epoch = 0
        self.device = device
        self.num_keypoints = num_keypoints
        self.img_height = img_height
        self.img_width = img_width
        self.gauss_sigma = gauss_sigma
        self.transform = transform
        self.return_uv = return_uv
        if instances is not None and not 1 <= int(instances) <= 16:
            raise ValueError("instances must be None or 1..16, got %r" % (instances,))
        self.instances = None if instances is None else int(instances)
        self.imgs = []
        self.labels = []
        self.labels_np = []           # host copies (DataLoader workers never touch the device)
        for i in range(len(os.listdir(labels_folder))):
            if self.instances is not None:
                label = self._load_instances(os.path.join(labels_folder, "%05d.npy" % i))
                self.imgs.append(os.path.join(img_folder, "%05d.jpg" % i))
                self.labels.append(torch.from_numpy(label).to(device))
                self.labels_np.append(label)
                continue
            label = np.load(os.path.join(labels_folder, "%05d.npy" % i)).reshape(num_keypoints, 2)
            if resize is None:
                label[:, 0] = np.clip(label[:, 0], 0, self.img_width - 1)      # dataset.py:65
                label[:, 1] = np.clip(label[:, 1], 0, self.img_height - 1)     # dataset.py:66
            self.imgs.append(os.path.join(img_folder, "%05d.jpg" % i))
            self.labels.append(torch.from_numpy(label).to(device))
            self.labels_np.append(label.astype(np.float32))

    def _load_instances(self, path):
        """One label file as float32 [K, M, 3], padded with empty slots (0, 0, 0)."""
        K, M = self.num_keypoints, self.instances
        a = np.load(path)
        if a.shape == (K, 2):
            a = np.concatenate([a, np.ones((K, 1), dtype=a.dtype)], 1)[:, None, :]
        elif a.shape == (K, 3):
            a = a[:, None, :]
        if a.ndim != 3 or a.shape[0] != K or a.shape[2] != 3 or not 1 <= a.shape[1] <= M:
            raise ValueError("%s: expected labels [%d,2], [%d,3] or [%d,m,3] with m <= %d, got %s"
                             % (path, K, K, K, M, a.shape))
        out = np.zeros((K, M, 3), dtype=np.float32)
        out[:, :a.shape[1]] = a
        if self.resize is None:
            out = self._mark_outside(out)
        return out

    def _mark_outside(self, pts):
        """Present points outside [0, w-1] x [0, h-1] lose their flag (not clipped)."""
        on = pts[..., 2] > 0
        with np.errstate(invalid="ignore"):
            inside = ((pts[..., 0] >= 0) & (pts[..., 0] <= self.img_width - 1) & (pts[..., 1] >= 0)
                      & (pts[..., 1] <= self.img_height - 1))
        pts = pts.copy()
        pts[..., 2] = np.where(on & ~inside, 0.0, pts[..., 2])
        return pts

    def set_epoch(self, epoch):
        """The epoch the geometric augmentation draws under (train.py's fit() calls it)."""
        self.epoch = int(epoch)

    def _decode(self, index):
        """(uint8 HWC image, [K,2] labels on the device), through `geometric` when set."""
        img = imread_bgr(self.imgs[index])
        if self.geometric is None and self.resize is None:
            return img, self.labels[index]
        uv = self.labels_np[index]
        if self.resize is not None:
            plan = self.resize.plan([img.shape[:2]], (self.img_height, self.img_width))
            flat = torch.from_numpy(np.ascontiguousarray(img).reshape(-1)).to(self.device)
            img = ops.resample_ragged_u8(flat, plan)[0].cpu().numpy()
            uv = (plan.apply_points(uv[None]) if self.instances is not None else plan.apply_uv(uv[None]))[0]
        if self.geometric is not None:
            if self.instances is not None:
                img, uv = self.geometric(img, pts=uv, index=index, epoch=self.epoch)
            else:
                img, uv = self.geometric(img, uv, index=index, epoch=self.epoch)
        return img, torch.from_numpy(uv).to(self.device)

    def __getitem__(self, index):
        img, labels = self._decode(index)
        img = self.transform(img)
        if self.return_uv:
            return img, labels.float()
        if self.instances is not None:
            pts = labels.float().unsqueeze(0).contiguous()
            return img, ops.gauss_target_multi(pts, self.img_height, self.img_width, self.gauss_sigma)[0]
        U = labels[:, 0]
        V = labels[:, 1]
        gaussians = gauss_2d_batch(self.img_width, self.img_height, self.gauss_sigma, U, V)
        return img, gaussians

    def raw(self, index):
        """(uint8 [H,W,3] BGR image as cv2.imread gives, fp32 [K,2] (u, v) on the device;
        with instances=M: fp32 [K,M,3] (u, v, flag))."""
        img, labels = self._decode(index)
        return img, labels.float()

    def __len__(self):
        return len(self.labels)


class SynthDataset(Dataset):
    """`length` procedural cable scenes of `scenes` (a hkp.synth.CableScenes) at hw = (h, w),
    rendered on the GPU; the labels are instance labels pts [K,M,3] (u, v, flag) with
    K = len(scenes.classes) and M = scenes.instances.  Item i of this rank is scene
    rank + i * world of the epoch set_epoch() gave (train.py's fit() calls it: new scenes
    every epoch); fixed=True ignores the epoch (a test set).  __getitem__ is the DataLoader
    idiom of train.py (keep num_workers=0): one image rendered by a B = 1 launch, through
    `transform`; items are (img, pts) with return_uv=True, else (img, gaussians) from
    hkp_gauss_target_multi.  raw(i) returns (uint8 [H,W,3] BGR on the host, fp32 [K,M,3]
    on the device).
    When the scenes have a line class (hkp.synth.LINE_CLASSES), and only then, the line
    labels lines [K,S,5] (hkp.lines) ride along: raw(i) and, with return_uv=True, the items
    are (img, pts, lines); with return_uv=False the gaussians are ops.line_target of the
    points and the segments together."""

    def __init__(self, scenes, length, hw, epoch=0, fixed=False, rank=0, world=1, transform=transform, return_uv=True,
                 device="cuda", gauss_sigma=8):
        if int(length) < 1 or int(world) < 1 or not 0 <= int(rank) < int(world):
            raise ValueError("SynthDataset: need length >= 1 and 0 <= rank < world, got %r, %r, %r"
                             % (length, rank, world))
        self.scenes, self.length = scenes, int(length)
        self.img_height, self.img_width = int(hw[0]), int(hw[1])
        self.num_keypoints, self.instances = len(scenes.classes), scenes.instances
        self.epoch, self.fixed, self.rank, self.world = int(epoch), bool(fixed), int(rank), int(world)
        self.transform, self.return_uv, self.device, self.gauss_sigma = transform, return_uv, device, gauss_sigma

    def __len__(self):
        return (self.length - self.rank + self.world - 1) // self.world

    def set_epoch(self, epoch):
        """The epoch the scenes are drawn under (ignored with fixed=True)."""
        if not self.fixed:
            self.epoch = int(epoch)

    def scene_index(self, i):
        if not 0 <= int(i) < len(self):
            raise IndexError(i)
        return self.rank + int(i) * self.world

    def plan(self, items, epoch=None):
        """The SynthPlan of dataset items `items` under `epoch` (None, or fixed=True: the
        dataset's own)."""
        e = self.epoch if epoch is None or self.fixed else int(epoch)
        return self.scenes.plan([self.scene_index(i) for i in items], e, (self.img_height, self.img_width))

    def raw(self, index):
        plan = self.plan([index])
        with torch.cuda.device(self.device):
            img = ops.synth_cables_u8(plan)[0].cpu().numpy()
        if plan.lines is not None:
            return img, torch.from_numpy(plan.pts[0]).to(self.device), torch.from_numpy(plan.lines[0]).to(self.device)
        return img, torch.from_numpy(plan.pts[0]).to(self.device)

    def __getitem__(self, index):
        got = self.raw(index)
        if len(got) == 3:                      # scenes with a line class
            from hkp import lines as L
            img, pts, lines = got
            img = self.transform(img)
            if self.return_uv:
                return img, pts, lines
            lab = L.concat(L.from_points(pts.unsqueeze(0)), lines.unsqueeze(0))
            return img, ops.line_target(lab, self.img_height, self.img_width, self.gauss_sigma)[0][0]
        img, pts = got
        img = self.transform(img)
        if self.return_uv:
            return img, pts
        return img, ops.gauss_target_multi(pts.unsqueeze(0).contiguous(), self.img_height, self.img_width,
                                           self.gauss_sigma)[0]


class _RawView(Dataset):
    """(uint8 [H,W,3] BGR, float32 [K,2]) host items of a KeypointsDataset — what
    DeviceBatches' decode workers produce."""

    def __init__(self, ds):
        self.paths, self.labels = ds.imgs, ds.labels_np

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, i):
        return imread_bgr(self.paths[i]), self.labels[i]


class _CoefView(Dataset):
    """Decode-worker items for DeviceBatches(decode="device"): the host half of the
    hybrid JPEG decode (hkp.jpeg.entropy_decode: quantised DCT coefficients and
    tables), or the host-decoded image for a file outside that decoder's subset."""

    def __init__(self, ds):
        self.paths, self.labels = ds.imgs, ds.labels_np

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, i):
        from hkp import jpeg
        path = self.paths[i]
        try:
            with open(path, "rb") as f:
                coefs, qt, g = jpeg.entropy_decode(f.read())
        except jpeg.JpegError:
            # outside the decoder's subset (JpegUnsupported) or damaged (a missing
            # RST marker, a bad Huffman code): the host decode, which like
            # cv2.imread (dataset.py:71) resyncs / zero-fills and still returns an
            # image, takes this file
            jpeg.host_lib()                  # ... but a missing library is a setup error, not a file's
            return ("img", imread_bgr(path), self.labels[i], path)
        return ("coef", (coefs, qt, bytes(g)), self.labels[i], path)


def _collate_coef(items):
    """One batch of _CoefView items: ("coef", coefs int16 [B,nblocks,64], qt
    [B,ncomp,64], geometry bytes, uv) when every image went through the entropy
    decoder with one geometry, else ("img", uint8 [B,H,W,3], uv) decoded on the host."""
    from hkp import jpeg
    uv = torch.from_numpy(np.stack([it[2] for it in items]))
    if all(it[0] == "coef" for it in items):
        geoms = [jpeg.Geom.from_buffer_copy(it[1][2]) for it in items]
        if all(g.key() == geoms[0].key() for g in geoms):
            coefs = torch.from_numpy(np.stack([it[1][0] for it in items]))
            qt = torch.from_numpy(np.stack([it[1][1] for it in items]).view(np.int16))
            return ("coef", coefs, qt, items[0][1][2], uv)
    imgs = [it[1] if it[0] == "img" else imread_bgr(it[3]) for it in items]
    return ("img", torch.from_numpy(np.stack(imgs)), uv)


def _collate_ragged(items):
    """One batch of _RawView items whose images may differ in size: ("ragged", flat
    uint8 [sum of H*W*3] with the images packed one after the other, int64 [B,2]
    (H, W) sizes, uv) — no np.stack."""
    imgs = [np.ascontiguousarray(it[0]) for it in items]
    sizes = np.array([im.shape[:2] for im in imgs], dtype=np.int64).reshape(-1, 2)
    flat = np.empty(int(sum(im.size for im in imgs)), dtype=np.uint8)
    off = 0
    for im in imgs:
        flat[off:off + im.size] = im.reshape(-1)
        off += im.size
    uv = torch.from_numpy(np.stack([it[1] for it in items]))
    return ("ragged", torch.from_numpy(flat), torch.from_numpy(sizes), uv)


def _collate_coef_ragged(items):
    """_collate_coef for DeviceBatches(resize=...): the "coef" batch when every image
    went through the entropy decoder with one geometry, else the host decode packed
    by _collate_ragged (the images may differ in size)."""
    from hkp import jpeg
    if all(it[0] == "coef" for it in items):
        g0 = jpeg.Geom.from_buffer_copy(items[0][1][2]).key()
        if all(jpeg.Geom.from_buffer_copy(it[1][2]).key() == g0 for it in items):
            return _collate_coef(items)
    return _collate_ragged([(it[1] if it[0] == "img" else imread_bgr(it[3]), it[2]) for it in items])


class _EpochBatches:
    """Batch sampler of the persistent decode loader: the current epoch's index
    batches (set by DeviceBatches before each epoch; iterated in the main process)."""

    def __init__(self):
        self.batches = []

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


def _collate_u8(items):
    imgs = torch.from_numpy(np.stack([it[0] for it in items]))
    uv = torch.from_numpy(np.stack([it[1] for it in items]))
    return imgs, uv


class DeviceBatches:
    """Iterate a KeypointsDataset as device batches (img uint8 [B,H,W,3], uv fp32
    [B,K,2]) for model.forward / Trainer.step(img, uv=uv).

    decode="host": images are decoded on the host (cv2 / PIL, as the reference).
    decode="device": the hybrid JPEG decode (hkp.jpeg) — the host only
    entropy-decodes the quantised DCT coefficients; they are copied (about the
    size of the decoded image) and the IDCT, upsampling and colour conversion run
    on the GPU on the copy stream, bit-identical to the host decode.  Files
    outside that decoder's subset (progressive, CMYK, ...) and batches of mixed
    geometry are decoded on the host instead.

    Host work runs in the calling thread (workers=0), or in `workers` DataLoader
    processes that decode and stack whole batches ahead (`prefetch` batches per
    worker) into pinned memory.  Each batch is copied with non_blocking=True on a
    side stream while the previous batch computes; the consumer's stream waits on
    an event.  `shuffle` uses a seeded permutation per epoch (train.py:61-67
    shuffles); batches come in order for any worker count.

    augment: a hkp.augment.DomainRandomization (dataset.py:18-31), or None.  When
    set, each batch is augmented on the copy stream right after its copy / JPEG
    reconstruct, image b under the program of (augment.seed, this epoch, its dataset
    index) — the same pixels for any batch size, worker count or decode mode.
    `augment` leaves the labels untouched (every one of its operators keeps the
    geometry).

    A dataset built with instances=M carries labels pts [K,M,3] (u, v, flag): the
    batches are then (img, pts fp32 [B,K,M,3]) for Trainer.step(img, pts=pts), and
    `geometric` / `resize` move them with plan.apply_points (a point that leaves the
    image becomes absent) instead of apply_uv.

    geometric: a hkp.geometry.GeometricAugmentation, or None.  When set, each batch is
    warped on the copy stream after its copy / JPEG reconstruct and before `augment`,
    image b under the transform of (geometric.seed, this epoch, its dataset index,
    its stored label), and the labels that are uploaded are plan.apply_uv(uv): moved
    by the same transform, flip pairs exchanged, clipped to the image.  The
    dataset's own `geometric` is not applied here (the decode workers read the raw
    files).

    resize: a hkp.resample.Resize, or None.  When set, the image files may have any
    size, also inside one batch: the decode workers hand the images over packed in
    one flat pinned buffer with their sizes, and the batch is resampled (antialiased,
    hkp_resample_u8, one launch) to the dataset's (img_height, img_width) on the copy
    stream right after its copy / JPEG reconstruct, before `geometric` and `augment`;
    the labels that go on are plan.apply_uv(uv).  Build the dataset with the same
    `resize`, so that its stored labels are in each file's own pixel coordinates.
    With decode="device" a batch of one JPEG geometry is reconstructed on the device
    and then resampled; a batch of mixed geometry takes the host decode.

    A SynthDataset takes a branch of its own: no workers, no host image, no copy.  Each
    batch is rendered on the copy stream by one hkp_synth_cables_u8 launch from the plan of
    (scenes, this epoch — the dataset's own with fixed=True —, its scene indices) and its
    pts uploaded from the plan;
    `geometric` and `augment` then apply exactly as for decoded batches, under the scene
    indices.  `resize` and decode="device" raise for it.  Scenes with a line class yield
    (img, pts, lines fp32 [B,K,S,5]) for Trainer.step(img, pts=pts, lines=lines); `geometric`
    moves the lines with plan.apply_lines (nothing is clipped or dropped)."""

    def __init__(self, dataset, batch_size, shuffle=False, seed=0, drop_last=False, device="cuda", workers=0,
                 prefetch=4, decode="host", augment=None, geometric=None, resize=None):
        if decode not in ("host", "device"):
            raise ValueError("decode must be 'host' or 'device', got %r" % (decode,))
        if isinstance(dataset, SynthDataset) and (resize is not None or decode != "host"):
            raise ValueError("DeviceBatches: a SynthDataset is rendered on the device at its own size: resize= and "
                             "decode='device' do not apply to it")
        self.ds, self.bs, self.shuffle, self.seed, self.drop_last = dataset, batch_size, shuffle, seed, drop_last
        self.device = torch.device(device)
        self.workers, self.prefetch, self.decode = workers, prefetch, decode
        self.augment = augment
        self.geometric = geometric
        self.resize = resize
        self.epoch = 0
        self._loader = None
        self._sampler = _EpochBatches()

    def __len__(self):
        n = len(self.ds)
        return n // self.bs if self.drop_last else (n + self.bs - 1) // self.bs

    def _view_collate(self):
        """The decode workers' dataset view and collate function."""
        if self.resize is not None:
            return ((_RawView(self.ds), _collate_ragged) if self.decode == "host"
                    else (_CoefView(self.ds), _collate_coef_ragged))
        return ((_RawView(self.ds), _collate_u8) if self.decode == "host" else (_CoefView(self.ds), _collate_coef))

    def _host_batches(self, batches):
        """Per index batch, in order: ("img", pinned uint8 [B,H,W,3], float32 [B,K,2])
        or (decode="device") ("coef", pinned coefs, pinned qt, geometry bytes, uv)."""
        view, collate = self._view_collate()
        if self.workers <= 0:
            for idx in batches:
                yield self._tag(collate([view[i] for i in idx]))
            return
        if self._loader is None:               # persistent workers: started once, reused every epoch
            from torch.utils.data import DataLoader
            self._loader = DataLoader(view, batch_sampler=self._sampler, num_workers=self.workers,
                                      collate_fn=collate, pin_memory=True, prefetch_factor=self.prefetch,
                                      persistent_workers=True)
        self._sampler.batches = [list(map(int, b)) for b in batches]
        for b in self._loader:
            yield self._tag(b)

    def _tag(self, b):
        """Host batches in one form, tensors pinned (the loader pins them already)."""
        if self.resize is not None:            # ("ragged", flat, sizes, uv) or ("coef", ...)
            return tuple(t.pin_memory() if torch.is_tensor(t) and not t.is_pinned() else t for t in b)
        if self.decode == "host":
            imgs, uv = b
            return ("img", imgs if imgs.is_pinned() else imgs.pin_memory(), uv)
        if b[0] == "img":
            return ("img", b[1] if b[1].is_pinned() else b[1].pin_memory(), b[2])
        return tuple(t.pin_memory() if torch.is_tensor(t) and not t.is_pinned() else t for t in b)

    def __iter__(self):
        n = len(self.ds)
        order = (np.random.default_rng(self.seed + self.epoch).permutation(n) if self.shuffle else np.arange(n))
        epoch = self.epoch
        self.epoch += 1
        batches = [order[i:i + self.bs] for i in range(0, n, self.bs)]
        if self.drop_last and batches and len(batches[-1]) < self.bs:
            batches.pop()
        copy_stream = torch.cuda.Stream(self.device)
        if isinstance(self.ds, SynthDataset):
            yield from self._synth_batches(batches, epoch, copy_stream)
            return
        host = self._host_batches(batches)
        staged = iter(batches)                 # host batches come in this order

        def stage():
            b = next(host)
            idx = next(staged)
            with torch.cuda.stream(copy_stream):
                rsizes = None
                if b[0] == "ragged":           # images of any size, packed: resampled below
                    buf, rsizes, uv = b[1], b[2].numpy(), b[3]
                    img = buf.to(self.device, non_blocking=True)
                elif b[0] == "img":
                    buf, uv = b[1], b[2]
                    img = buf.to(self.device, non_blocking=True)
                else:                          # hybrid decode: coefficients up, pixels made on the device
                    from hkp import jpeg
                    _, coefs, qt, gbytes, uv = b
                    buf = (coefs, qt)
                    g = jpeg.Geom.from_buffer_copy(gbytes)
                    img = jpeg.reconstruct(coefs.to(self.device, non_blocking=True),
                                           qt.to(self.device, non_blocking=True), g, coefs.shape[0])
                if self.resize is not None:
                    if rsizes is None:         # a reconstructed batch: one size
                        rsizes = [(img.shape[1], img.shape[2])] * img.shape[0]
                    rplan = self.resize.plan(rsizes, (self.ds.img_height, self.ds.img_width))
                    img = ops.resample_ragged_u8(img.reshape(-1), rplan)
                    uv = (rplan.apply_points(uv) if uv.dim() == 4 else rplan.apply_uv(uv)).pin_memory()
                    buf = (buf, rplan, uv)     # the plan's pinned records and tables live as long as the batch's
                if self.geometric is not None:
                    gplan = self.geometric.plan(idx, epoch, uvs=uv, hw=(img.shape[1], img.shape[2]))
                    img = ops.warp_affine_u8(img, gplan)
                    uv = (gplan.apply_points(uv) if uv.dim() == 4 else gplan.apply_uv(uv)).pin_memory()
                    buf = (buf, gplan, uv)     # the plan's pinned records and the labels live as long as the batch's
                if self.augment is not None:
                    plan = self.augment.plan(idx, epoch)
                    img = ops.augment_u8(img, plan)
                    buf = (buf, plan)          # the plan's pinned arrays live as long as the batch's
                uvd = uv.to(self.device, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(copy_stream)
            return img, uvd, ev, buf

        nxt = stage() if batches else None
        for bi in range(len(batches)):
            img, uv, ev, buf = nxt
            nxt = stage() if bi + 1 < len(batches) else None
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(ev)
            img.record_stream(cur)
            uv.record_stream(cur)
            yield img, uv

    def _synth_batches(self, batches, epoch, copy_stream):
        """__iter__ for a SynthDataset: render, warp and augment on the copy stream, one
        batch ahead of the consumer."""
        ds = self.ds

        def stage(items):
            idx = [ds.scene_index(i) for i in items]
            with torch.cuda.device(self.device), torch.cuda.stream(copy_stream):
                plan = ds.plan(items, epoch)
                img = ops.synth_cables_u8(plan)
                pts = torch.from_numpy(plan.pts)
                lines = None if plan.lines is None else torch.from_numpy(plan.lines)
                buf = plan                     # the plan's pinned records live as long as the batch
                if self.geometric is not None:
                    gplan = self.geometric.plan(idx, epoch, uvs=pts, hw=(img.shape[1], img.shape[2]))
                    img = ops.warp_affine_u8(img, gplan)
                    pts = gplan.apply_points(pts)
                    if lines is not None:
                        lines = gplan.apply_lines(lines)
                    buf = (buf, gplan)
                if self.augment is not None:
                    aplan = self.augment.plan(idx, epoch)
                    img = ops.augment_u8(img, aplan)
                    buf = (buf, aplan)
                pts = pts.pin_memory()
                ptsd = pts.to(self.device, non_blocking=True)
                linesd = None
                if lines is not None:           # scenes with a line class
                    lines = lines.pin_memory()
                    linesd = lines.to(self.device, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(copy_stream)
            return img, ptsd, linesd, ev, (buf, pts, lines)

        nxt = stage(batches[0]) if batches else None
        for bi in range(len(batches)):
            img, pts, lines, ev, buf = nxt
            nxt = stage(batches[bi + 1]) if bi + 1 < len(batches) else None
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(ev)
            img.record_stream(cur)
            pts.record_stream(cur)
            if lines is None:
                yield img, pts
            else:
                lines.record_stream(cur)
                yield img, pts, lines
