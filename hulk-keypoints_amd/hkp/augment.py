"""Domain randomisation on the GPU for uint8 [B,H,W,3] BGR batches: the reference's
commented-out imgaug pipeline (dataset.py:18-31) as programs for hkp_augment_u8.

The host samples each image's parameters and folds every transcendental into
small tables (per-channel 256-entry LUTs, the three blur weights, one Gaussian
quantile table); the kernel (csrc/augment.hip) does table look-ups and plainly
rounded fp32 arithmetic only, so tests/_augment_ref.py restates it in numpy bit
for bit.  Pixel parity with imgaug itself is NOT pinned (imgaug is not
installed and its source is not in the reference); README lists the deliberate
deviations.  There is no CPU path.

  operator       reference augmenter (dataset.py)                    stage
  hue_sat        AddToHueAndSaturation((-20, 20))            :21     HSV
  contrast       LinearContrast((0.85, 1.2), per_channel=0.25) :22   LUT
  add            Add((-10, 30), per_channel=True)            :23     LUT
  gamma          GammaContrast((0.85, 1.2))                  :24     LUT
  blur           GaussianBlur(sigma=(0.0, 0.6))              :25     BLUR
  temperature    ChangeColorTemperature((5000, 35000))       :26     LUT
  mul_sat        MultiplySaturation((0.95, 1.05))            :27     HSV
  noise          AdditiveGaussianNoise(scale=(0, 0.0125*255)) :28    NOISE
"""
import ctypes
import math
import statistics

import numpy as np
import torch

from ._lib import (HKP_AUG_BLUR, HKP_AUG_GAUSS_TABLE, HKP_AUG_HSV, HKP_AUG_LUT, HKP_AUG_MAX_STAGES, HKP_AUG_NOISE,
                   HKP_AUG_TILE_H, HKP_AUG_TILE_W, AugProgram, HkpError)

TILE_H, TILE_W = HKP_AUG_TILE_H, HKP_AUG_TILE_W       # one block's tile (csrc/augment.hip)

# the reference's operators in its listed order, with its parameter ranges
OPERATORS = ("hue_sat", "contrast", "add", "gamma", "blur", "temperature", "mul_sat", "noise")
RANGES = {"hue_sat": (-20, 20), "contrast": (0.85, 1.2), "add": (-10, 30), "gamma": (0.85, 1.2), "blur": (0.0, 0.6),
          "temperature": (5000, 35000), "mul_sat": (0.95, 1.05), "noise": (0.0, 0.0125 * 255)}
CONTRAST_PER_CHANNEL = 0.25
BLUR_MIN_SIGMA = 0.001        # below: the stage is dropped


# ------------------------------------------------------------------ tables ----
def _lut(values):
    """float64 values [..., 256] → uint8 (rint half to even, clamp)."""
    return np.clip(np.rint(values), 0, 255).astype(np.uint8)


def lut_contrast(alphas):
    """LinearContrast: out = 127 + alpha_c * (v - 127); alphas in memory order (B, G, R)."""
    v = np.arange(256, dtype=np.float64)
    return _lut(np.stack([127.0 + float(a) * (v - 127.0) for a in alphas]))


def lut_add(adds):
    """Add: out = v + a_c."""
    v = np.arange(256, dtype=np.float64)
    return _lut(np.stack([v + float(a) for a in adds]))


def lut_gamma(gamma):
    """GammaContrast: out = 255 * (v / 255) ** gamma."""
    v = np.arange(256, dtype=np.float64)
    t = 255.0 * (v / 255.0) ** float(gamma)
    return _lut(np.stack([t, t, t]))


def kelvin_multipliers(kelvin):
    """(m_R, m_G, m_B) of a blackbody at `kelvin`: Tanner Helland's fit, each value
    clamped to [0, 255] and divided by 255 (imgaug's own kelvin table is not
    available, so this is a stated deviation)."""
    t = float(kelvin) / 100.0
    if t <= 66.0:
        r = 255.0
        g = 99.4708025861 * math.log(t) - 161.1195681661
        b = 138.5177312231 * math.log(t - 10.0) - 305.0447927307 if t > 10.0 else 0.0
    else:
        r = 329.698727446 * (t - 60.0) ** -0.1332047592
        g = 288.1221695283 * (t - 60.0) ** -0.0755148492
        b = 255.0
    return tuple(min(max(c, 0.0), 255.0) / 255.0 for c in (r, g, b))


def lut_temperature(kelvin):
    """ChangeColorTemperature: out_c = v * m_c(T); rows in memory order (B, G, R)."""
    m_r, m_g, m_b = kelvin_multipliers(kelvin)
    v = np.arange(256, dtype=np.float64)
    return _lut(np.stack([v * m_b, v * m_g, v * m_r]))


def blur_weights(sigma):
    """(w0, w1, w2) fp32 of the 5-tap Gaussian: exp(-k^2 / 2 sigma^2) in float64,
    normalised so that w0 + 2 w1 + 2 w2 = 1."""
    s = float(sigma)
    w = [math.exp(-(k * k) / (2.0 * s * s)) for k in range(3)]
    tot = w[0] + 2.0 * w[1] + 2.0 * w[2]
    return tuple(np.float32(x / tot) for x in w)


_gauss_host = None
_gauss_dev = {}


def gauss_table():
    """fp32 [4096]: T[i] = Phi^-1((i + 0.5) / 4096), the quantile table the NOISE
    stage indexes with the top 12 bits of a Philox word (a Gaussian truncated at
    +-3.67 sigma, variance 0.99968)."""
    global _gauss_host
    if _gauss_host is None:
        nd = statistics.NormalDist()
        n = HKP_AUG_GAUSS_TABLE
        _gauss_host = np.array([nd.inv_cdf((i + 0.5) / n) for i in range(n)], dtype=np.float64).astype(np.float32)
        _gauss_host.setflags(write=False)
    return _gauss_host


class GaussTable:
    """Handle of the quantile table: `.host` (numpy) and `.on(device)`, uploaded once
    per device."""

    @property
    def host(self):
        return gauss_table()

    def on(self, device):
        device = torch.device(device)
        key = device.index if device.index is not None else torch.cuda.current_device()
        t = _gauss_dev.get(key)
        if t is None:
            t = torch.from_numpy(gauss_table().copy()).to(torch.device("cuda", key))
            torch.cuda.current_stream(t.device).synchronize()    # once: later streams find it complete
            _gauss_dev[key] = t
        return t


TABLE = GaussTable()


# ------------------------------------------------------------------- plans ----
class Plan:
    """The packed host arrays of one batch: `programs` (ctypes AugProgram * n), `luts`
    (uint8 [n, HKP_AUG_MAX_STAGES, 3, 256]; slot i belongs to stage i) and `table`
    (the Gaussian table handle).  device_arrays() uploads programs and luts from
    pinned memory on the current stream; the plan keeps the pinned and the device
    copies alive, so keep the plan until the batch has been consumed."""

    def __init__(self, programs, luts):
        self.programs, self.luts, self.table = programs, luts, TABLE
        self.n = len(programs)
        self._dev = {}

    @classmethod
    def from_stages(cls, per_image):
        """per_image: for each image a list of stages
             ("lut", uint8 [3, 256])   ("hsv", dh, add, mul)
             ("blur", w0, w1, w2)      ("noise", scale, key0, key1)"""
        n = len(per_image)
        programs = (AugProgram * n)()
        luts = np.zeros((n, HKP_AUG_MAX_STAGES, 3, 256), dtype=np.uint8)
        for b, stages in enumerate(per_image):
            if len(stages) > HKP_AUG_MAX_STAGES:
                raise HkpError("augment: a program holds at most %d stages, got %d" % (HKP_AUG_MAX_STAGES, len(stages)))
            p = programs[b]
            p.nstages = len(stages)
            for i, st in enumerate(stages):
                s = p.stages[i]
                if st[0] == "lut":
                    t = np.asarray(st[1])
                    if t.shape != (3, 256) or t.dtype != np.uint8:
                        raise HkpError("augment: a LUT stage takes a uint8 [3, 256] table")
                    s.kind = HKP_AUG_LUT
                    luts[b, i] = t
                elif st[0] == "hsv":
                    s.kind = HKP_AUG_HSV
                    s.f[0], s.f[1], s.f[2] = float(st[1]), float(st[2]), float(st[3])
                elif st[0] == "blur":
                    s.kind = HKP_AUG_BLUR
                    s.f[0], s.f[1], s.f[2] = float(st[1]), float(st[2]), float(st[3])
                elif st[0] == "noise":
                    s.kind = HKP_AUG_NOISE
                    s.f[0] = float(st[1])
                    s.key[0], s.key[1] = int(st[2]) & 0xFFFFFFFF, int(st[3]) & 0xFFFFFFFF
                else:
                    raise HkpError("augment: unknown stage %r" % (st[0],))
            if sum(1 for st in stages if st[0] == "blur") > 1:
                raise HkpError("augment: a program holds at most one BLUR stage")
        return cls(programs, luts)

    def program_bytes(self):
        """The programs as a numpy uint8 view [n, sizeof(AugProgram)] (shares memory)."""
        return np.frombuffer(self.programs, dtype=np.uint8).reshape(self.n, ctypes.sizeof(AugProgram))

    def device_arrays(self, device):
        device = torch.device(device)
        key = device.index if device.index is not None else torch.cuda.current_device()
        got = self._dev.get(key)
        if got is None:
            dev = torch.device("cuda", key)
            pin_p = torch.from_numpy(self.program_bytes().copy()).pin_memory()
            pin_l = torch.from_numpy(self.luts).pin_memory()
            got = (pin_p.to(dev, non_blocking=True), pin_l.to(dev, non_blocking=True), pin_p, pin_l)
            self._dev[key] = got
        return got[0], got[1]


# ---------------------------------------------------------------- sampling ----
class DomainRandomization:
    """The reference's domain-randomisation transform (dataset.py:18-31) for the
    device data path.

    seed          with (epoch, sample_index) it fixes a sample's program: the program
                  does not depend on batch size, batch composition, worker count or rank.
    random_order  iaa.Sequential(..., random_order=True): a fresh permutation of the
                  operators per sample; False keeps the listed order.
    ops           None: the reference's eight operators and ranges.  A list of names
                  selects a subset (in that order).  A dict overrides ranges, e.g.
                  {"noise": (0, 0)}; a value of None drops that operator.

    Draw order (part of the contract), from
    numpy.random.default_rng([seed, epoch, sample_index]):
      1. random_order only: permutation(len(operators)) — position → operator;
      2. per operator, in the LISTED order (so parameters do not depend on the
         permutation):
           hue_sat      integers(lo, hi + 1)
           contrast     random() (per channel iff < 0.25), then uniform(lo, hi, 3)
                        (always three draws; shared: the first for all channels)
           add          integers(lo, hi + 1, 3)
           gamma, blur, temperature, mul_sat, noise      uniform(lo, hi)
      3. the NOISE key: integers(0, 2**32, 2) — always drawn.
    Channel triples are in memory order (B, G, R).

    Called with a uint8 [B,H,W,3] or [H,W,3] device tensor, or a numpy HWC uint8
    image, it returns the same kind (the numpy image is uploaded, augmented on the
    GPU and copied back), so Compose([DomainRandomization(...), _to_tensor]) is the
    drop-in for the reference's commented transform.  Such calls number their images
    0, 1, 2, ... as sample indices under `self.epoch` (default 0); DeviceBatches
    (augment=...) uses the dataset's indices and its own epoch instead."""

    def __init__(self, seed=0, random_order=True, ops=None):
        self.seed, self.random_order = int(seed), bool(random_order)
        ranges = dict(RANGES)
        names = list(OPERATORS)
        if isinstance(ops, dict):
            for k, v in ops.items():
                if k not in RANGES:
                    raise ValueError("unknown operator %r (known: %s)" % (k, ", ".join(OPERATORS)))
                if v is None:
                    names.remove(k)
                else:
                    ranges[k] = (v[0], v[1])
        elif ops is not None:
            names = list(ops)
            for k in names:
                if k not in RANGES:
                    raise ValueError("unknown operator %r (known: %s)" % (k, ", ".join(OPERATORS)))
            if len(set(names)) != len(names):
                raise ValueError("an operator may be listed once")
        self.operators, self.ranges = tuple(names), ranges
        self.epoch = 0
        self._calls = 0

    def sample(self, index, epoch=0):
        """The parameters of sample `index` in `epoch`: a dict with "order" (operator
        names in application order), one entry per operator, "contrast_per_channel"
        and "key"."""
        rng = np.random.default_rng([self.seed, int(epoch), int(index)])
        ops = self.operators
        order = [ops[i] for i in rng.permutation(len(ops))] if self.random_order else list(ops)
        p = {"order": order}
        for name in ops:
            lo, hi = self.ranges[name]
            if name == "hue_sat":
                p[name] = int(rng.integers(int(lo), int(hi) + 1))
            elif name == "contrast":
                per = bool(rng.random() < CONTRAST_PER_CHANNEL)
                a = rng.uniform(lo, hi, 3)
                p["contrast_per_channel"] = per
                p[name] = tuple(float(x) for x in a) if per else (float(a[0]),) * 3
            elif name == "add":
                p[name] = tuple(int(x) for x in rng.integers(int(lo), int(hi) + 1, 3))
            else:
                p[name] = float(rng.uniform(lo, hi))
        p["key"] = tuple(int(x) for x in rng.integers(0, 2 ** 32, 2, dtype=np.uint64))
        return p

    @staticmethod
    def stages(p):
        """The stage list (Plan.from_stages) of sampled parameters `p`."""
        out = []
        for name in p["order"]:
            v = p[name]
            if name == "hue_sat":
                out.append(("hsv", np.float32(6.0 * v / 255.0), float(v), 1.0))
            elif name == "contrast":
                out.append(("lut", lut_contrast(v)))
            elif name == "add":
                out.append(("lut", lut_add(v)))
            elif name == "gamma":
                out.append(("lut", lut_gamma(v)))
            elif name == "temperature":
                out.append(("lut", lut_temperature(v)))
            elif name == "mul_sat":
                out.append(("hsv", 0.0, 0.0, np.float32(v)))
            elif name == "blur":
                if v >= BLUR_MIN_SIGMA:
                    out.append(("blur",) + blur_weights(v))
            elif name == "noise":
                if v != 0.0:
                    out.append(("noise", np.float32(v), p["key"][0], p["key"][1]))
        return out

    def plan(self, indices, epoch=0):
        """The Plan of one batch: sample `indices[b]` of `epoch` for image b."""
        return Plan.from_stages([self.stages(self.sample(int(i), epoch)) for i in indices])

    def __call__(self, img):
        if torch.utils.data.get_worker_info() is not None:
            raise HkpError("DomainRandomization runs on the GPU and DataLoader workers never touch the device: "
                           "keep num_workers=0 for this transform, or use DeviceBatches(augment=...) "
                           "with decode workers")
        from . import ops
        is_np = isinstance(img, np.ndarray)
        if is_np:
            if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
                raise HkpError("DomainRandomization: expected a uint8 [H,W,3] image, got %s %s"
                               % (img.dtype, img.shape))
            x = torch.from_numpy(np.ascontiguousarray(img)).to("cuda")
        elif isinstance(img, torch.Tensor):
            x = img
        else:
            raise HkpError("DomainRandomization: expected a numpy image or a device tensor, got %s" % type(img))
        single = x.dim() == 3
        if single:
            x = x.unsqueeze(0)
        n = x.shape[0] if x.dim() == 4 else 0
        plan = self.plan(range(self._calls, self._calls + n), self.epoch)
        out = ops.augment_u8(x, plan)
        self._calls += n
        if single:
            out = out[0]
        # (the plan may go now: its device arrays are reused in stream order, and the host
        # allocator holds pinned blocks until the copies queued from them are done)
        return out.cpu().numpy() if is_np else out
