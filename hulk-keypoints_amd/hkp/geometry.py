"""Geometric augmentation and resize on the GPU for uint8 [B,H,W,3] batches:
host-side matrix builders over one kernel, hkp_warp_affine_u8 (csrc/warp.hip), a
batched per-image affine warp.  The labels travel through the same transform.

Conventions
  * Integer pixel coordinates are pixel centres, as for the labels (u, v) and
    hkp_gauss_target.  A forward matrix M (2x3, float64) maps source to dest:
    (u', v') = M @ (u, v, 1).  The kernel reads the INVERSE map, quantised to Q16
    (quantize_inverse), and does integer arithmetic only (include/hulkkp.h), so
    tests/_warp_ref.py restates it in numpy bit for bit.
  * A positive rotate_deg turns the picture counter-clockwise on the screen (y
    points down): +90 on a square image equals numpy.rot90(img, 1).
  * Parity with cv2.warpAffine or imgaug's Affine is NOT pinned (neither is
    installed): their fixed-point formats and rounding differ from the ones
    here.  The reference has no geometric augmentation at all; the sampling
    ranges below are this project's own.  There is no CPU path.
"""
import math

import numpy as np
import torch

from ._lib import (HKP_WARP_BILINEAR, HKP_WARP_BORDER_CONSTANT, HKP_WARP_BORDER_REFLECT101, HKP_WARP_BORDER_REPLICATE,
                   HKP_WARP_MAX_DIM, HKP_WARP_NEAREST, HkpError, WarpXform)

INTERP = {"bilinear": HKP_WARP_BILINEAR, "nearest": HKP_WARP_NEAREST}
BORDER = {"constant": HKP_WARP_BORDER_CONSTANT, "replicate": HKP_WARP_BORDER_REPLICATE,
          "reflect101": HKP_WARP_BORDER_REFLECT101}
Q = 65536.0          # Q16


# ---------------------------------------------------------------- matrices ----
def affine_matrix(h, w, rotate_deg=0.0, scale=1.0, translate_xy_px=(0.0, 0.0), shear_deg=0.0, hflip=False,
                  vflip=False):
    """The forward 2x3 matrix (source -> dest, float64) of an h x w image, composed
    about the image centre c = ((w-1)/2, (h-1)/2):

        M = T(translate) . T(c) . R(rotate) . S(scale) . Shear_x(shear) . Flip . T(-c)

    flips innermost, translation outermost.  R turns counter-clockwise on the
    screen for a positive angle; Shear_x is [[1, tan(shear)], [0, 1]]."""
    t = math.radians(float(rotate_deg))
    c, s = math.cos(t), math.sin(t)
    R = np.array([[c, s], [-s, c]], dtype=np.float64)
    S = np.eye(2) * float(scale)
    Sh = np.array([[1.0, math.tan(math.radians(float(shear_deg)))], [0.0, 1.0]])
    F = np.diag([-1.0 if hflip else 1.0, -1.0 if vflip else 1.0])
    A = R @ S @ Sh @ F
    ctr = np.array([(w - 1) / 2.0, (h - 1) / 2.0])
    M = np.empty((2, 3), dtype=np.float64)
    M[:, :2] = A
    M[:, 2] = ctr + np.asarray(translate_xy_px, dtype=np.float64) - A @ ctr
    return M


def resize_matrix(hs, ws, h, w):
    """Forward matrix of the resize hs x ws -> h x w with half-pixel centres: its
    inverse is src = (dst + 0.5) * ws / w - 0.5 (and the same for rows)."""
    fx, fy = float(w) / float(ws), float(h) / float(hs)
    return np.array([[fx, 0.0, 0.5 * fx - 0.5], [0.0, fy, 0.5 * fy - 0.5]], dtype=np.float64)


def quantize_inverse(M):
    """The six Q16 int32 coefficients of the inverse (dest -> source) of forward
    matrix M, row major: inverted in float64, rint(inv * 65536).  HkpError for a
    singular matrix or a coefficient outside int32."""
    M = np.asarray(M, dtype=np.float64)
    if M.shape != (2, 3):
        raise HkpError("quantize_inverse: expected a 2x3 matrix, got %s" % (M.shape,))
    a, b, d, e = M[0, 0], M[0, 1], M[1, 0], M[1, 1]
    det = a * e - b * d
    if not np.all(np.isfinite(M)) or abs(det) <= 1e-12 * max(1.0, float(np.abs(M[:, :2]).max()) ** 2):
        raise HkpError("quantize_inverse: the matrix is singular (det %g)" % det)
    inv = np.array([[e, -b], [-d, a]], dtype=np.float64) / det
    full = np.empty((2, 3), dtype=np.float64)
    full[:, :2] = inv
    full[:, 2] = -inv @ M[:, 2]
    q = np.rint(full * Q).reshape(6)
    if np.any(np.abs(q) >= 2.0 ** 31):
        raise HkpError("quantize_inverse: a Q16 coefficient does not fit int32 (largest %g)" % np.abs(q).max())
    return q.astype(np.int32)


def transform_uv(M, uv):
    """Forward matrix M applied to keypoints uv [..., 2] (u = column, v = row) in
    float64; float32 result."""
    M = np.asarray(M, dtype=np.float64)
    p = np.asarray(uv, dtype=np.float64)
    return (p @ M[:, :2].T + M[:, 2]).astype(np.float32)


def swap_pairs(uv, pairs):
    """uv [K, 2] with keypoint rows a and b exchanged for every (a, b) of `pairs`
    (left / right landmarks of a flipped image); a copy."""
    out = np.array(uv, copy=True)
    for a, b in pairs:
        out[[a, b]] = out[[b, a]]
    return out


# ------------------------------------------------------------------- plans ----
class WarpPlan:
    """One batch of transforms: `xforms` (ctypes WarpXform * n, the quantised inverse
    maps and fill colours), `matrices` (float64 [n, 2, 3], forward), `flipped` (bool
    [n]: an odd number of flips), `flip_pairs`, `hw` (output size), `interp` and
    `border` (HKP_WARP_*).  device_array() uploads the records from pinned memory on
    the current stream; the plan keeps the pinned and the device copy alive, so keep
    the plan until the batch has been consumed."""

    def __init__(self, matrices, hw, flipped=None, flip_pairs=(), fill=(0, 0, 0), interp="bilinear",
                 border="constant"):
        mats = np.asarray(matrices, dtype=np.float64)
        if mats.ndim != 3 or mats.shape[1:] != (2, 3) or mats.shape[0] < 1:
            raise HkpError("WarpPlan: expected forward matrices [n, 2, 3], got %s" % (mats.shape,))
        if interp not in INTERP:
            raise HkpError("WarpPlan: unknown interp %r (known: %s)" % (interp, ", ".join(INTERP)))
        if border not in BORDER:
            raise HkpError("WarpPlan: unknown border %r (known: %s)" % (border, ", ".join(BORDER)))
        if len(fill) != 3 or any(int(f) != f or not 0 <= f <= 255 for f in fill):
            raise HkpError("WarpPlan: fill is three integers in 0..255 (B, G, R), got %r" % (fill,))
        self.n = mats.shape[0]
        self.matrices = mats
        self.hw = (int(hw[0]), int(hw[1]))
        self.flipped = np.zeros(self.n, dtype=bool) if flipped is None else np.asarray(flipped, dtype=bool).reshape(self.n)
        self.flip_pairs = tuple((int(a), int(b)) for a, b in flip_pairs)
        self.interp, self.border = INTERP[interp], BORDER[border]
        self.xforms = (WarpXform * self.n)()
        for b in range(self.n):
            q = quantize_inverse(mats[b])
            for i in range(6):
                self.xforms[b].m[i] = int(q[i])
            for i in range(3):
                self.xforms[b].fill[i] = int(fill[i])
        self._dev = {}

    def xform_bytes(self):
        """The records as a numpy uint8 view [n, 32] (shares memory)."""
        return np.frombuffer(self.xforms, dtype=np.uint8).reshape(self.n, 32)

    def coefficients(self):
        """int32 [n, 6]: the quantised inverse maps (a copy)."""
        return np.array([[x.m[i] for i in range(6)] for x in self.xforms], dtype=np.int32)

    def device_array(self, device):
        device = torch.device(device)
        key = device.index if device.index is not None else torch.cuda.current_device()
        got = self._dev.get(key)
        if got is None:
            pin = torch.from_numpy(self.xform_bytes().copy()).pin_memory()
            got = (pin.to(torch.device("cuda", key), non_blocking=True), pin)
            self._dev[key] = got
        return got[0]

    def mask_lut(self, device):
        """uint8 [n, 256] on `device`, or None when no image needs a table: hkp.masks.flip_lut
        of `flip_pairs` for the flipped images, the identity for the others.  Uploaded from
        pinned memory on the current stream and cached on the plan like device_array()."""
        if not self.flip_pairs or not self.flipped.any():
            return None
        device = torch.device(device)
        key = ("lut", device.index if device.index is not None else torch.cuda.current_device())
        got = self._dev.get(key)
        if got is None:
            from .masks import flip_lut
            ident, swap = flip_lut(()), flip_lut(self.flip_pairs)
            pin = torch.stack([swap if f else ident for f in self.flipped]).pin_memory()
            got = (pin.to(torch.device("cuda", key[1]), non_blocking=True), pin)
            self._dev[key] = got
        return got[0]

    def apply_mask(self, mask, fill=0):
        """An ignore mask (hkp.masks: uint8 [n, Hs, Ws] class bits, on the device) through
        the batch's transforms -> uint8 [n, h, w] in the warped images' frame
        (ops.warp_mask_u8).  The plan's matrices and border are used; `interp` is not: a mask
        is always sampled nearest.  Where the image was flipped, the class bits of
        `flip_pairs` are exchanged, as apply_points exchanges the label rows.  fill: the byte
        outside the source under border="constant" (0: trained, 255: ignored)."""
        from . import ops
        if not isinstance(mask, torch.Tensor):
            raise HkpError("apply_mask: expected a uint8 tensor [%d, H, W] on the device" % self.n)
        return ops.warp_mask_u8(mask, self, fill=fill, lut=self.mask_lut(mask.device))

    def apply_uv(self, uv):
        """Labels through the batch's transforms: uv [n, K, 2] on the host (numpy or
        a CPU tensor; the same kind comes back, float32) -> forward matrix, rows of
        `flip_pairs` exchanged where the image was flipped an odd number of times,
        then clipped to [0, w-1] x [0, h-1] (the reference's label rule,
        dataset.py:65-66)."""
        is_t = isinstance(uv, torch.Tensor)
        a = uv.detach().cpu().numpy() if is_t else np.asarray(uv)
        if a.ndim != 3 or a.shape[0] != self.n or a.shape[2] != 2:
            raise HkpError("apply_uv: expected labels [%d, K, 2], got %s" % (self.n, a.shape))
        out = np.empty(a.shape, dtype=np.float32)
        for b in range(self.n):
            p = transform_uv(self.matrices[b], a[b])
            out[b] = swap_pairs(p, self.flip_pairs) if self.flipped[b] else p
        h, w = self.hw
        out[..., 0] = np.clip(out[..., 0], 0, w - 1)
        out[..., 1] = np.clip(out[..., 1], 0, h - 1)
        return torch.from_numpy(out) if is_t else out

    def apply_points(self, pts):
        """Instance labels through the batch's transforms: pts [n, K, M, 3] on the host
        (u, v, flag; numpy or a CPU tensor, the same kind comes back, float32).  (u, v)
        of the present slots (flag > 0) go through the forward matrix, rows of
        `flip_pairs` are exchanged along K (whole [M, 3] rows) where the image was
        flipped, and a present point that leaves [0, w-1] x [0, h-1] — the range
        apply_uv clips to — gets flag 0; it is not clipped.  Empty slots pass through
        as they are."""
        is_t, a = host_points(pts, self.n, "apply_points")
        out = np.array(a, dtype=np.float32, copy=True)
        h, w = self.hw
        for b in range(self.n):
            on = out[b, :, :, 2] > 0
            q = transform_uv(self.matrices[b], np.where(on[..., None], out[b, :, :, :2], 0.0))
            inside = (q[..., 0] >= 0) & (q[..., 0] <= w - 1) & (q[..., 1] >= 0) & (q[..., 1] <= h - 1)
            out[b, :, :, :2] = np.where(on[..., None], q, out[b, :, :, :2])
            out[b, :, :, 2] = np.where(on & ~inside, 0.0, out[b, :, :, 2])
            if self.flipped[b]:
                out[b] = swap_pairs(out[b], self.flip_pairs)
        return torch.from_numpy(out) if is_t else out

    def apply_lines(self, lines):
        """Line labels through the batch's transforms: lines [n, K, S, 5] on the host
        (x0, y0, x1, y1, flag; numpy or a CPU tensor, the same kind comes back, float32).
        Both ends of the present slots (flag > 0) go through the forward matrix, as
        apply_points' (u, v) do, and rows of `flip_pairs` are exchanged along K where the
        image was flipped.  Nothing is clipped or dropped: the affine image of a segment
        is the segment between the images of its ends, and the distance to it is defined
        for every pixel.  Empty slots pass through as they are."""
        is_t, a = host_lines(lines, self.n, "apply_lines")
        out = np.array(a, dtype=np.float32, copy=True)
        for b in range(self.n):
            on = (out[b, :, :, 4] > 0)[..., None]
            for e in (0, 2):
                q = transform_uv(self.matrices[b], np.where(on, out[b, :, :, e:e + 2], 0.0))
                out[b, :, :, e:e + 2] = np.where(on, q, out[b, :, :, e:e + 2])
            if self.flipped[b]:
                out[b] = swap_pairs(out[b], self.flip_pairs)
        return torch.from_numpy(out) if is_t else out


def host_lines(lines, n, who):
    """(is a tensor, numpy view) of line labels [n, K, S, 5] on the host."""
    is_t = isinstance(lines, torch.Tensor)
    a = lines.detach().cpu().numpy() if is_t else np.asarray(lines)
    if a.ndim != 4 or a.shape[0] != n or a.shape[3] != 5:
        raise HkpError("%s: expected line labels [%d, K, S, 5], got %s" % (who, n, a.shape))
    return is_t, a


def host_points(pts, n, who):
    """(is a tensor, numpy view) of instance labels [n, K, M, 3] on the host."""
    is_t = isinstance(pts, torch.Tensor)
    a = pts.detach().cpu().numpy() if is_t else np.asarray(pts)
    if a.ndim != 4 or a.shape[0] != n or a.shape[3] != 3:
        raise HkpError("%s: expected instance labels [%d, K, M, 3], got %s" % (who, n, a.shape))
    return is_t, a


# ---------------------------------------------------------------- sampling ----
class GeometricAugmentation:
    """Rotation, scale, translation, shear and flips for the device data path, image
    and labels together.  The reference has no geometric augmentation: the operators
    and the default ranges are this project's own choice (a common setting for
    keypoint heat-map training), not the reference's.

    seed        with (epoch, sample_index) it fixes a sample's transform: it does not
                depend on batch size, batch composition, worker count or rank.
    rotate      degrees (lo, hi), counter-clockwise on the screen.
    scale       factor (lo, hi) about the image centre.
    translate   (lo, hi) as a fraction of the width (x) and of the height (y).
    shear       degrees (lo, hi), x-shear.
    hflip, vflip  probabilities.  flip_pairs: keypoint rows to exchange when an image
                was flipped an odd number of times (left / right landmarks).
    fill        (B, G, R) of border="constant"; border: "constant", "replicate" or
                "reflect101"; interp: "bilinear" or "nearest".
    keep_inside with labels given: up to `tries` parameter sets are drawn and the first
                whose transformed keypoints all lie inside the image is taken, else the
                identity.  Without labels the first draw is taken.

    Draw order (part of the contract), from
    numpy.random.default_rng([seed, epoch, sample_index, 1]) (the trailing word keeps
    the stream apart from DomainRandomization's under the same seed); per try, always
    all of them, whatever the ranges:
      1. rotate      uniform(lo, hi)
      2. scale       uniform(lo, hi)
      3. translate   uniform(lo, hi, 2)  — x fraction, y fraction
      4. shear       uniform(lo, hi)
      5. flips       random(2) — hflip iff [0] < hflip, vflip iff [1] < vflip
    Try t + 1 continues the same generator after try t.

    Called with a uint8 [B,H,W,3] or [H,W,3] device tensor, or a numpy HWC uint8
    image, it returns the same kind; with uv ([B,K,2] / [K,2], numpy or tensor) it
    returns (img, uv) with the labels transformed, swapped and clipped.  Such calls
    number their images 0, 1, 2, ... as sample indices under `self.epoch` unless
    `index` (an int, or one per image) and `epoch` are given; DeviceBatches
    (geometric=...) and KeypointsDataset(geometric=...) pass the dataset's indices."""

    def __init__(self, seed=0, rotate=(-30, 30), scale=(0.9, 1.1), translate=(-0.1, 0.1), shear=(0, 0), hflip=0.0,
                 vflip=0.0, flip_pairs=(), fill=(0, 0, 0), border="constant", interp="bilinear", keep_inside=True,
                 tries=8):
        self.seed = int(seed)
        for name, r in (("rotate", rotate), ("scale", scale), ("translate", translate), ("shear", shear)):
            if len(r) != 2 or not float(r[0]) <= float(r[1]):
                raise ValueError("%s must be (lo, hi) with lo <= hi, got %r" % (name, r))
        if not float(scale[0]) > 0:
            raise ValueError("scale must be positive, got %r" % (scale,))
        if not (0.0 <= hflip <= 1.0 and 0.0 <= vflip <= 1.0):
            raise ValueError("hflip and vflip are probabilities")
        if interp not in INTERP or border not in BORDER:
            raise ValueError("unknown interp %r or border %r" % (interp, border))
        if int(tries) < 1:
            raise ValueError("tries must be at least 1")
        self.rotate, self.scale = (float(rotate[0]), float(rotate[1])), (float(scale[0]), float(scale[1]))
        self.translate, self.shear = (float(translate[0]), float(translate[1])), (float(shear[0]), float(shear[1]))
        self.hflip, self.vflip = float(hflip), float(vflip)
        self.flip_pairs = tuple((int(a), int(b)) for a, b in flip_pairs)
        self.fill, self.border, self.interp = tuple(int(f) for f in fill), border, interp
        self.keep_inside, self.tries = bool(keep_inside), int(tries)
        self.epoch = 0
        self._calls = 0

    def _draw(self, rng):
        p = {"rotate": float(rng.uniform(*self.rotate)), "scale": float(rng.uniform(*self.scale))}
        t = rng.uniform(self.translate[0], self.translate[1], 2)
        p["translate"] = (float(t[0]), float(t[1]))
        p["shear"] = float(rng.uniform(*self.shear))
        f = rng.random(2)
        p["hflip"], p["vflip"] = bool(f[0] < self.hflip), bool(f[1] < self.vflip)
        return p

    @staticmethod
    def matrix(p, hw):
        """The forward matrix of sampled parameters `p` for an image of size hw."""
        h, w = hw
        return affine_matrix(h, w, p["rotate"], p["scale"], (p["translate"][0] * w, p["translate"][1] * h),
                             p["shear"], p["hflip"], p["vflip"])

    def sample(self, index, epoch=0, uv=None, hw=None, pts=None):
        """The parameters of sample `index` in `epoch`: a dict with "rotate", "scale",
        "translate" (fractions), "shear", "hflip", "vflip" and "try" (which draw was
        taken; -1: the identity, after `tries` draws left a keypoint outside).  uv
        [K, 2] and hw = (h, w) switch the keep_inside search on; so do instance labels
        pts [K, M, 3] (u, v, flag) in place of uv, of which only the present slots
        (flag > 0) are tested.  The draws are the same either way."""
        if uv is not None and pts is not None:
            raise HkpError("GeometricAugmentation.sample: pass uv or pts, not both")
        rng = np.random.default_rng([self.seed, int(epoch), int(index), 1])
        if (uv is None and pts is None) or not self.keep_inside:
            p = self._draw(rng)
            p["try"] = 0
            return p
        if hw is None:
            raise HkpError("GeometricAugmentation.sample: keep_inside with labels needs hw=(h, w)")
        h, w = hw
        if pts is not None:
            rec = np.asarray(pts).reshape(-1, 3)
            uv = rec[rec[:, 2] > 0, :2]
        pts = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
        for t in range(self.tries):
            p = self._draw(rng)
            q = transform_uv(self.matrix(p, hw), pts)
            if np.all((q[:, 0] >= 0) & (q[:, 0] <= w - 1) & (q[:, 1] >= 0) & (q[:, 1] <= h - 1)):
                p["try"] = t
                return p
        return {"rotate": 0.0, "scale": 1.0, "translate": (0.0, 0.0), "shear": 0.0, "hflip": False, "vflip": False,
                "try": -1}

    def plan(self, indices, epoch=0, uvs=None, hw=None, pts=None):
        """The WarpPlan of one batch: sample `indices[b]` of `epoch` for image b of
        size hw = (h, w); uvs [B, K, 2] (host), or instance labels pts [B, K, M, 3] in
        their place (also accepted as uvs), feeds keep_inside."""
        if hw is None:
            raise HkpError("GeometricAugmentation.plan: hw=(h, w) is required")
        indices = [int(i) for i in indices]
        if uvs is not None and pts is None and np.ndim(uvs) == 4:
            uvs, pts = None, uvs
        if pts is not None:
            if uvs is not None:
                raise HkpError("GeometricAugmentation.plan: pass uvs or pts, not both")
            _, pa = host_points(pts, len(indices), "GeometricAugmentation.plan")
            ps = [self.sample(i, epoch, hw=hw, pts=pa[b]) for b, i in enumerate(indices)]
            plan = WarpPlan([self.matrix(p, hw) for p in ps], hw, flipped=[p["hflip"] != p["vflip"] for p in ps],
                            flip_pairs=self.flip_pairs, fill=self.fill, interp=self.interp, border=self.border)
            plan.params = ps
            return plan
        if uvs is not None:
            uvs = uvs.detach().cpu().numpy() if isinstance(uvs, torch.Tensor) else np.asarray(uvs)
            if uvs.ndim != 3 or uvs.shape[0] != len(indices) or uvs.shape[2] != 2:
                raise HkpError("GeometricAugmentation.plan: expected labels [%d, K, 2], got %s"
                               % (len(indices), uvs.shape))
        ps = [self.sample(i, epoch, None if uvs is None else uvs[b], hw) for b, i in enumerate(indices)]
        plan = WarpPlan([self.matrix(p, hw) for p in ps], hw, flipped=[p["hflip"] != p["vflip"] for p in ps],
                        flip_pairs=self.flip_pairs, fill=self.fill, interp=self.interp, border=self.border)
        plan.params = ps
        return plan

    def __call__(self, img, uv=None, index=None, epoch=None, pts=None):
        """pts ([B,K,M,3] / [K,M,3] instance labels: u, v, flag) in place of uv: (img, pts)
        comes back, the labels through WarpPlan.apply_points."""
        if uv is not None and pts is not None:
            raise HkpError("GeometricAugmentation: pass uv or pts, not both")
        is_pts = pts is not None
        if is_pts:
            uv = pts
        if torch.utils.data.get_worker_info() is not None:
            raise HkpError("GeometricAugmentation runs on the GPU and DataLoader workers never touch the device: "
                           "keep num_workers=0 for this transform, or use DeviceBatches(geometric=...) "
                           "with decode workers")
        from . import ops
        is_np = isinstance(img, np.ndarray)
        if is_np:
            if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
                raise HkpError("GeometricAugmentation: expected a uint8 [H,W,3] image, got %s %s"
                               % (img.dtype, img.shape))
            x = torch.from_numpy(np.ascontiguousarray(img)).to("cuda")
        elif isinstance(img, torch.Tensor):
            x = img
        else:
            raise HkpError("GeometricAugmentation: expected a numpy image or a device tensor, got %s" % type(img))
        single = x.dim() == 3
        if single:
            x = x.unsqueeze(0)
        if x.dim() != 4 or x.shape[3] != 3:
            raise HkpError("GeometricAugmentation: expected [B,H,W,3] or [H,W,3], got %s" % (tuple(img.shape),))
        n, h, w = x.shape[0], x.shape[1], x.shape[2]
        uv_t = isinstance(uv, torch.Tensor)
        uv_a = None
        if uv is not None:
            uv_a = (uv.detach().cpu().numpy() if uv_t else np.asarray(uv)).astype(np.float32)
            squeeze = single and uv_a.ndim == (3 if is_pts else 2)
            if squeeze:
                uv_a = uv_a[None]
        if index is None:
            indices = range(self._calls, self._calls + n)
            self._calls += n
        else:
            indices = [int(index)] if np.ndim(index) == 0 else [int(i) for i in index]
        plan = self.plan(indices, self.epoch if epoch is None else epoch, uvs=None if is_pts else uv_a,
                         pts=uv_a if is_pts else None, hw=(h, w))
        out = ops.warp_affine_u8(x, plan)
        if single:
            out = out[0]
        # (the plan may go now: its device array is reused in stream order, and the host
        # allocator holds pinned blocks until the copies queued from them are done)
        out = out.cpu().numpy() if is_np else out
        if uv is None:
            return out
        new = plan.apply_points(uv_a) if is_pts else plan.apply_uv(uv_a)
        if squeeze:
            new = new[0]
        return out, (torch.from_numpy(new).to(uv.device) if uv_t else new)
