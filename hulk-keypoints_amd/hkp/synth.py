"""Procedural cable scenes: labelled training data from a seed.  The scene model and
the sampler live here; one kernel, hkp_synth_cables_u8 (csrc/synth.hip), renders a
batch of scenes as uint8 [B,H,W,3] BGR straight into the device data path, and the
labels come from the scene description itself, in the instance format pts [B,K,M,3]
(u, v, flag) the loss and the metrics speak.

Conventions
  * Integer pixel coordinates are pixel centres, as for the labels and
    hkp_gauss_target.  Geometry is float64 on the host; the kernel reads it in fixed
    point (quantize_piece; include/hulkkp.h is the definition) and does integer
    arithmetic only, so tests/_synth_ref.py restates it in numpy bit for bit.
  * A scene is a function of (seed, epoch, index) and hw alone: batch size, batch
    order and worker count do not enter.
  * Pieces are drawn in table order, later over earlier: blobs, then the cables piece
    by piece in cable order (the over / under at a crossing), then the caps.
  * Realism is NOT pinned: the reference's authors rendered their data from a cable
    simulator; this is a seeded stand-in that gives every layer above it an exact
    ground truth.  There is no CPU path.
"""

import numpy as np
import torch

from ._lib import (HKP_LINE_MAX_S, HKP_SYNTH_MAX_DIM, HKP_SYNTH_MAX_SEGS, MAX_INSTANCES, HkpError, SynthScene,
                   SynthSeg)

CLASSES = ("cap", "tail", "crossing", "blob")
LINE_CLASSES = ("cable",)          # labelled by segments (hkp.lines), not by points
DEFAULT_BACKGROUND = {"bg0": (40, 40, 40), "bg1": (96, 96, 96), "key": (0, 0), "cell_log2": 5}


# ------------------------------------------------------------- geometry ----
def catmull_rom(ctrl, segments):
    """The uniform Catmull-Rom curve through control points ctrl [n, 2] (n >= 2, the end
    points doubled as phantom neighbours), at segments + 1 evenly spaced parameters:
    float64 [segments + 1, 2].  The first and the last vertex are the end control points."""
    p = np.asarray(ctrl, dtype=np.float64)
    n = p.shape[0]
    q = np.concatenate([p[:1], p, p[-1:]], 0)
    t = np.linspace(0.0, n - 1.0, int(segments) + 1)
    i = np.minimum(t.astype(np.int64), n - 2)
    f = (t - i)[:, None]
    p0, p1, p2, p3 = q[i], q[i + 1], q[i + 2], q[i + 3]
    out = 0.5 * (2.0 * p1 + (p2 - p0) * f + (2.0 * p0 - 5.0 * p1 + 4.0 * p2 - p3) * f * f
                 + (3.0 * p1 - p0 - 3.0 * p2 + p3) * f * f * f)
    out[0], out[-1] = p[0], p[-1]
    return out


def fit_into(poly, lo, hi):
    """poly [n, 2] with each axis whose extent leaves [lo, hi] mapped linearly onto the part
    of its extent inside (an axis that is inside stays as it is)."""
    out = np.array(poly, dtype=np.float64, copy=True)
    for a in (0, 1):
        mn, mx = out[:, a].min(), out[:, a].max()
        nlo, nhi = max(mn, lo[a]), min(mx, hi[a])
        if (mn < lo[a] or mx > hi[a]) and mx > mn:
            out[:, a] = nlo + (out[:, a] - mn) * ((nhi - nlo) / (mx - mn))
        out[:, a] = np.clip(out[:, a], lo[a], hi[a])
    return out


def crossings(polys):
    """Intersections of the centrelines of polylines (list of [n, 2] float64): every pair of
    pieces except a piece with itself and with its neighbours on the same polyline, each
    piece half open (its end vertex belongs to the next).  Returns (points [c, 2], angles
    [c] in degrees, 0..90, ids [c, 4]: polyline and piece of the two strands)."""
    a0 = np.concatenate([p[:-1] for p in polys], 0)
    a1 = np.concatenate([p[1:] for p in polys], 0)
    pid = np.concatenate([np.full(len(p) - 1, k) for k, p in enumerate(polys)])
    sid = np.concatenate([np.arange(len(p) - 1) for p in polys])
    r = a1 - a0
    n = len(a0)
    i, j = np.triu_indices(n, 1)
    keep = ~((pid[i] == pid[j]) & (np.abs(sid[i] - sid[j]) <= 1))
    i, j = i[keep], j[keep]
    den = r[i, 0] * r[j, 1] - r[i, 1] * r[j, 0]
    w = a0[j] - a0[i]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (w[:, 0] * r[j, 1] - w[:, 1] * r[j, 0]) / den
        u = (w[:, 0] * r[i, 1] - w[:, 1] * r[i, 0]) / den
    hit = (den != 0) & (t >= 0) & (t < 1) & (u >= 0) & (u < 1)
    i, j, t = i[hit], j[hit], t[hit]
    pts = a0[i] + t[:, None] * r[i]
    cos = np.abs((r[i] * r[j]).sum(1)) / np.maximum(np.hypot(*r[i].T) * np.hypot(*r[j].T), 1e-300)
    ang = np.degrees(np.arccos(np.clip(cos, 0.0, 1.0)))
    return pts, ang, np.stack([pid[i], sid[i], pid[j], sid[j]], 1).reshape(-1, 4)


def point_polyline_distance(pt, poly, first=0, last=None):
    """Distance of point pt to the pieces first .. last - 1 of polyline poly (inf: none)."""
    a, b = poly[:-1][first:last], poly[1:][first:last]
    if len(a) == 0:
        return np.inf
    d = b - a
    l2 = np.maximum((d * d).sum(1), 1e-300)
    t = np.clip(((pt - a) * d).sum(1) / l2, 0.0, 1.0)
    c = a + t[:, None] * d - pt
    return float(np.sqrt((c * c).sum(1)).min())


# ---------------------------------------------------------- fixed point ----
def quantize_piece(p0, p1, radius, bgr, shade, arc):
    """One capsule from p0 to p1 (pixels, float64; p1 == p0: a disc) as the fields of
    hkp_synth_seg: vertices rounded to Q4, the direction and the length taken between the
    ROUNDED vertices (so neighbouring pieces share their joint), direction rint(. * 2^14),
    radius rint(. * 16) and the constants that follow from it."""
    x0, y0 = int(np.rint(p0[0] * 16.0)), int(np.rint(p0[1] * 16.0))
    x1, y1 = int(np.rint(p1[0] * 16.0)), int(np.rint(p1[1] * 16.0))
    ln = float(np.hypot(x1 - x0, y1 - y0))
    if ln > 0:
        ux, uy, qlen = int(np.rint((x1 - x0) / ln * 16384.0)), int(np.rint((y1 - y0) / ln * 16384.0)), int(np.rint(ln))
    else:
        ux, uy, qlen = 16384, 0, 0
    r = int(np.rint(float(radius) * 16.0))
    if not 16 <= r <= 512:
        raise HkpError("synth: radius %g px outside 1..32 px" % float(radius))
    if max(abs(x0), abs(y0)) > 1 << 17 or qlen > 1 << 18:
        raise HkpError("synth: a piece from %r to %r leaves the kernel's coordinate range (+-8192 px)" % (p0, p1))
    if not 0 <= int(shade) <= 256:
        raise HkpError("synth: shade %r outside 0..256" % (shade,))
    ri, ro, r2 = (r - 8) ** 2, (r + 8) ** 2, r * r
    return {"x0": x0, "y0": y0, "ux": ux, "uy": uy, "len": qlen, "r": r, "r_in2": ri, "r_out2": ro, "r2": r2,
            "inv": (1 << 32) // (ro - ri), "inv_r2": (1 << 32) // r2, "bgr": tuple(int(c) for c in bgr),
            "shade": int(shade), "arc": int(arc)}


def _colour(c, what):
    if len(c) != 3 or any(int(v) != v or not 0 <= v <= 255 for v in c):
        raise HkpError("synth: %s is three integers in 0..255 (B, G, R), got %r" % (what, c))
    return tuple(int(v) for v in c)


# ----------------------------------------------------------------- plans ----
class SynthPlan:
    """One batch of scenes for hkp_synth_cables_u8: `scenes` (ctypes SynthScene * n) and
    `segs` (ctypes SynthSeg * nsegs, the piece table in the kernel's fixed point), `hw`,
    `pts` (float32 [n, K, M, 3] labels, or None for a plan built from bare geometry),
    `lines` (float32 [n, K, S, 5] line labels, or None when no class is a line class),
    `fallback` (bool [n]) and `descs` (the float64 scene descriptions, when sampled).
    device_arrays() uploads the records from pinned memory on the current stream; the plan
    keeps the pinned and the device copies alive, so keep it until the batch has been
    consumed.

    pieces: per image a list of quantize_piece() dicts in drawing order; backgrounds: per
    image a dict with "bg0", "bg1" (B, G, R), "key" (two uint32) and "cell_log2" (4..12)."""

    def __init__(self, hw, pieces, backgrounds, pts=None, fallback=None, descs=None, lines=None):
        h, w = int(hw[0]), int(hw[1])
        if not (1 <= h <= HKP_SYNTH_MAX_DIM and 1 <= w <= HKP_SYNTH_MAX_DIM):
            raise HkpError("SynthPlan: hw %dx%d outside 1..%d" % (h, w, HKP_SYNTH_MAX_DIM))
        if len(pieces) < 1 or len(pieces) != len(backgrounds):
            raise HkpError("SynthPlan: need one piece list and one background per image")
        self.n, self.hw = len(pieces), (h, w)
        self.nsegs = max(1, sum(len(p) for p in pieces))
        self.scenes = (SynthScene * self.n)()
        self.segs = (SynthSeg * self.nsegs)()
        off = 0
        for b, (ps, bg) in enumerate(zip(pieces, backgrounds)):
            if len(ps) > HKP_SYNTH_MAX_SEGS:
                raise HkpError("SynthPlan: image %d has %d pieces (at most %d)" % (b, len(ps), HKP_SYNTH_MAX_SEGS))
            sc = self.scenes[b]
            sc.seg_off, sc.seg_cnt, sc.cell_log2 = off, len(ps), int(bg["cell_log2"])
            if not 4 <= sc.cell_log2 <= 12:
                raise HkpError("SynthPlan: cell_log2 %d outside 4..12" % sc.cell_log2)
            sc.key[0], sc.key[1] = int(bg["key"][0]) & 0xFFFFFFFF, int(bg["key"][1]) & 0xFFFFFFFF
            for c, (v0, v1) in enumerate(zip(_colour(bg["bg0"], "bg0"), _colour(bg["bg1"], "bg1"))):
                sc.bg0[c], sc.bg1[c] = v0, v1
            for p in ps:
                s = self.segs[off]
                for f in ("x0", "y0", "ux", "uy", "len", "r", "r_in2", "r_out2", "r2", "inv", "inv_r2", "shade", "arc"):
                    setattr(s, f, p[f])
                for c in range(3):
                    s.bgr[c] = p["bgr"][c]
                off += 1
        self.pts = None if pts is None else np.ascontiguousarray(pts, dtype=np.float32)
        self.lines = None if lines is None else np.ascontiguousarray(lines, dtype=np.float32)
        self.fallback = np.zeros(self.n, dtype=bool) if fallback is None else np.asarray(fallback, dtype=bool)
        self.descs = descs
        self._dev = {}

    @classmethod
    def from_polylines(cls, hw, polylines, radii, colours, background=None, shades=None):
        """A plan from explicit geometry, without the sampler or its rules.  polylines: per
        image a list of float [n, 2] vertex arrays in pixels (n == 1: a disc), drawn in list
        order, each its own arc; radii (pixels) and colours ((B, G, R)) and, optionally,
        shades (0..256, default 96) are lists of the same shape.  background: one dict for
        every image or a list of dicts (DEFAULT_BACKGROUND's keys; missing keys take its
        values).  No labels: pts is None."""
        n = len(polylines)
        bgs = background if isinstance(background, (list, tuple)) else [background] * n
        bgs = [dict(DEFAULT_BACKGROUND, **(bg or {})) for bg in bgs]
        pieces = []
        for b in range(n):
            ps = []
            for k, poly in enumerate(polylines[b]):
                v = np.asarray(poly, dtype=np.float64).reshape(-1, 2)
                sh = 96 if shades is None else shades[b][k]
                col = _colour(colours[b][k], "a colour")
                ends = [(v[0], v[0])] if len(v) == 1 else zip(v[:-1], v[1:])
                ps += [quantize_piece(p0, p1, radii[b][k], col, sh, k) for p0, p1 in ends]
            pieces.append(ps)
        return cls(hw, pieces, bgs)

    def scene_bytes(self):
        """The scene records as a numpy uint8 view [n, 64] (shares memory)."""
        return np.frombuffer(self.scenes, dtype=np.uint8).reshape(self.n, 64)

    def seg_bytes(self):
        """The piece table as a numpy uint8 view [nsegs, 64] (shares memory)."""
        return np.frombuffer(self.segs, dtype=np.uint8).reshape(self.nsegs, 64)

    def device_arrays(self, device):
        """(scenes, segs) on `device`, copied once per device from pinned memory."""
        device = torch.device(device)
        key = device.index if device.index is not None else torch.cuda.current_device()
        got = self._dev.get(key)
        if got is None:
            pins = (torch.from_numpy(self.scene_bytes().copy()).pin_memory(),
                    torch.from_numpy(self.seg_bytes().copy()).pin_memory())
            dev = torch.device("cuda", key)
            got = (pins[0].to(dev, non_blocking=True), pins[1].to(dev, non_blocking=True), pins)
            self._dev[key] = got
        return got[0], got[1]


# -------------------------------------------------------------- sampling ----
class CableScenes:
    """Seeded scenes of cables on a noise background, image and labels together.

    seed        with (epoch, index) it fixes a scene.
    classes     the label planes and their order, out of "cap" (the capped end of each
                cable: vertex 0), "tail" (the other end), "crossing" (intersections of the
                centrelines, a cable with itself or with another, neighbouring pieces
                excluded) and "blob" (the disc centres), and out of LINE_CLASSES: "cable"
                (the centrelines themselves, labelled by their pieces: line_labels; its
                row of the point labels is empty); K = len(classes).
    cables      (lo, hi) cables per scene; ctrl: (lo, hi) control points per cable;
                segments: straight pieces per cable; radius: (lo, hi) pixels.
    blobs       (lo, hi) filled discs per scene (distractors, and the easy class), of
                radius blob_radius (lo, hi) pixels.
    min_sep     two labelled points of one class are at least this far apart (pixels).
    min_angle   a crossing is at least this steep (degrees).
    tries       candidates per scene; after that many the fallback scene is taken: one
                straight cable between opposite corners of the margin box, no blobs.
    instances   M, the slots per label plane: a candidate with more of a class is redrawn.
    margin      the cables and blob centres stay this far inside the picture (pixels);
                None: 1.5 * radius[1] + 4, which keeps every cap inside.

    A candidate is redrawn while any of these holds: two labelled points of one class
    closer than min_sep; a crossing shallower than min_angle; more than M instances of a
    class; a labelled end within (its cable's radius + the strand's radius + 2 px) of a
    strand's centreline, its own neighbourhood aside (the pieces of its own cable up to
    the first vertex farther than 2 * radius + 2 px from the end); a blob centre within
    (its radius + the cable's radius) of a cable's centreline.

    Draw order (part of the contract), try t from
    numpy.random.default_rng([seed, epoch, index, t, 2]) (the trailing word keeps the
    stream apart from DomainRandomization's and GeometricAugmentation's under one seed):
      1. background  integers(24, 112, 3) bg0; integers(8, 72, 3) added to it: bg1;
                     integers(0, 2^32, 2) key; integers(4, 7) cell_log2
      2. blobs       integers(lo, hi + 1) their number; per blob uniform(0, 1, 2) centre in
                     the margin box, uniform(*blob_radius), integers(64, 256, 3) colour,
                     integers(32, 129) shade
      3. cables      integers(lo, hi + 1) their number; per cable integers(lo, hi + 1)
                     control points, uniform(0, 1, [n, 2]) in the margin box,
                     uniform(*radius), integers(48, 256, 3) colour, integers(48, 256, 3) cap
                     colour, integers(64, 193) shade
    The fallback scene draws 1. and one cable's radius, colours and shade from try `tries`."""

    def __init__(self, seed=0, classes=CLASSES, cables=(1, 2), ctrl=(3, 5), segments=48, radius=(4.0, 8.0),
                 blobs=(0, 3), min_sep=16.0, min_angle=20.0, tries=32, instances=8, blob_radius=(6.0, 14.0),
                 margin=None):
        self.seed = int(seed)
        self.classes = tuple(classes)
        known = CLASSES + LINE_CLASSES
        if not self.classes or any(c not in known for c in self.classes) or len(set(self.classes)) != len(self.classes):
            raise ValueError("classes must be distinct names out of %r, got %r" % (known, classes))
        for name, r, lo in (("cables", cables, 1), ("ctrl", ctrl, 2), ("blobs", blobs, 0)):
            if len(r) != 2 or int(r[0]) != r[0] or int(r[1]) != r[1] or not lo <= r[0] <= r[1]:
                raise ValueError("%s must be integers (lo, hi) with %d <= lo <= hi, got %r" % (name, lo, r))
        for name, r in (("radius", radius), ("blob_radius", blob_radius)):
            if len(r) != 2 or not 1.0 <= float(r[0]) <= float(r[1]) or 1.5 * float(r[1]) > 32.0:
                raise ValueError("%s must be (lo, hi) pixels with 1 <= lo <= hi and 1.5 * hi <= 32, got %r" % (name, r))
        if int(segments) < 1 or int(tries) < 1:
            raise ValueError("segments and tries must be at least 1")
        if not 1 <= int(instances) <= MAX_INSTANCES:
            raise ValueError("instances must be 1..%d, got %r" % (MAX_INSTANCES, instances))
        if int(blobs[1]) + int(cables[1]) * (int(segments) + 1) > HKP_SYNTH_MAX_SEGS:
            raise ValueError("blobs + cables * (segments + 1) must not exceed %d pieces" % HKP_SYNTH_MAX_SEGS)
        self.line_slots = int(cables[1]) * int(segments) if any(c in LINE_CLASSES for c in self.classes) else 0
        if self.line_slots > HKP_LINE_MAX_S:
            raise ValueError("a line class needs cables[1] * segments = %d segment slots (at most %d)"
                             % (self.line_slots, HKP_LINE_MAX_S))
        self.cables, self.ctrl, self.blobs = tuple(map(int, cables)), tuple(map(int, ctrl)), tuple(map(int, blobs))
        self.segments, self.tries, self.instances = int(segments), int(tries), int(instances)
        self.radius, self.blob_radius = tuple(map(float, radius)), tuple(map(float, blob_radius))
        self.min_sep, self.min_angle = float(min_sep), float(min_angle)
        self.margin = 1.5 * self.radius[1] + 4.0 if margin is None else float(margin)
        self.epoch = 0
        self._calls = 0

    # -- one candidate ---------------------------------------------------------
    def _box(self, hw):
        h, w = hw
        m = self.margin
        if w - 1 - 2 * m < 1 or h - 1 - 2 * m < 1:
            raise HkpError("CableScenes: a %dx%d picture leaves no room inside a margin of %g px" % (h, w, m))
        return np.array([m, m]), np.array([w - 1 - m, h - 1 - m])

    @staticmethod
    def _background(rng):
        bg0 = rng.integers(24, 112, 3)
        bg1 = bg0 + rng.integers(8, 72, 3)
        key = rng.integers(0, 1 << 32, 2)
        return {"bg0": tuple(int(v) for v in bg0), "bg1": tuple(int(v) for v in bg1),
                "key": (int(key[0]), int(key[1])), "cell_log2": int(rng.integers(4, 7))}

    def _cable_look(self, rng):
        return {"radius": float(rng.uniform(*self.radius)), "colour": tuple(int(v) for v in rng.integers(48, 256, 3)),
                "cap_colour": tuple(int(v) for v in rng.integers(48, 256, 3)), "shade": int(rng.integers(64, 193))}

    def _draw(self, rng, hw):
        lo, hi = self._box(hw)
        d = {"background": self._background(rng), "blobs": [], "cables": []}
        for _ in range(int(rng.integers(self.blobs[0], self.blobs[1] + 1))):
            c = lo + rng.uniform(0.0, 1.0, 2) * (hi - lo)
            d["blobs"].append({"centre": c, "radius": float(rng.uniform(*self.blob_radius)),
                               "colour": tuple(int(v) for v in rng.integers(64, 256, 3)),
                               "shade": int(rng.integers(32, 129))})
        for _ in range(int(rng.integers(self.cables[0], self.cables[1] + 1))):
            nc = int(rng.integers(self.ctrl[0], self.ctrl[1] + 1))
            ctrl = lo + rng.uniform(0.0, 1.0, (nc, 2)) * (hi - lo)
            cab = {"poly": fit_into(catmull_rom(ctrl, self.segments), lo, hi)}
            cab.update(self._cable_look(rng))
            d["cables"].append(cab)
        return d

    def _fallback(self, rng, hw):
        lo, hi = self._box(hw)
        t = np.linspace(0.0, 1.0, self.segments + 1)[:, None]
        d = {"background": self._background(rng), "blobs": [], "cables": [{"poly": lo + t * (hi - lo)}]}
        d["cables"][0].update(self._cable_look(rng))
        return d

    def label_points(self, d):
        """The labelled points of scene description d, per class name: float64 [c, 2]; the
        crossings' angles ride along under "_angles"."""
        polys = [c["poly"] for c in d["cables"]]
        x, ang, _ = crossings(polys)
        return {"cap": np.array([p[0] for p in polys]).reshape(-1, 2),
                "tail": np.array([p[-1] for p in polys]).reshape(-1, 2), "crossing": x,
                "blob": np.array([b["centre"] for b in d["blobs"]]).reshape(-1, 2), "_angles": ang}

    def broken_rule(self, d, lab=None):
        """The first validity rule scene d breaks, as a string, or None."""
        lab = self.label_points(d) if lab is None else lab
        for c in CLASSES:
            p = lab[c]
            if len(p) > self.instances:
                return "more than %d instances of %s" % (self.instances, c)
            if len(p) > 1:
                dd = np.hypot(*(p[:, None, :] - p[None, :, :]).transpose(2, 0, 1))
                if dd[np.triu_indices(len(p), 1)].min() < self.min_sep:
                    return "two %s points closer than min_sep" % c
        if len(lab["_angles"]) and lab["_angles"].min() < self.min_angle:
            return "a crossing shallower than min_angle"
        for ci, cab in enumerate(d["cables"]):
            poly, r = cab["poly"], cab["radius"]
            for end in (0, -1):
                pt = poly[end]
                far = np.hypot(*(poly - pt).T) > 2.0 * r + 2.0
                # own neighbourhood: the pieces up to the first vertex that is far from the end
                idx = np.nonzero(far if end == 0 else far[::-1])[0]
                own = int(idx[0]) if len(idx) else len(poly) - 1
                for cj, other in enumerate(d["cables"]):
                    first, last = 0, None
                    if cj == ci:
                        first, last = (own, None) if end == 0 else (0, len(poly) - 1 - own)
                    if point_polyline_distance(pt, other["poly"], first, last) < r + other["radius"] + 2.0:
                        return "an end under a strand"
        for b in d["blobs"]:
            for cab in d["cables"]:
                if point_polyline_distance(b["centre"], cab["poly"]) < b["radius"] + cab["radius"]:
                    return "a blob centre under a cable"
        return None

    def sample(self, index, epoch=0, hw=None):
        """The scene description of scene `index` in `epoch` for a picture of size hw = (h, w):
        a dict with "background", "blobs", "cables" (each with its float64 "poly"), "labels"
        (per class name, float64 [c, 2]), "try" (which candidate was taken) and "fallback"."""
        if hw is None:
            raise HkpError("CableScenes.sample: hw=(h, w) is required")
        hw = (int(hw[0]), int(hw[1]))
        for t in range(self.tries):
            d = self._draw(np.random.default_rng([self.seed, int(epoch), int(index), t, 2]), hw)
            lab = self.label_points(d)
            if self.broken_rule(d, lab) is None:
                d.update(labels=lab, fallback=False)
                d["try"] = t
                return d
        d = self._fallback(np.random.default_rng([self.seed, int(epoch), int(index), self.tries, 2]), hw)
        d.update(labels=self.label_points(d), fallback=True)
        d["try"] = self.tries
        return d

    def pieces(self, d):
        """Scene description d as quantize_piece() dicts in drawing order: blobs, cables,
        caps (discs of 1.5 * radius at vertex 0)."""
        ps, arc = [], 0
        for b in d["blobs"]:
            ps.append(quantize_piece(b["centre"], b["centre"], b["radius"], b["colour"], b["shade"], arc))
            arc += 1
        for cab in d["cables"]:
            v = cab["poly"]
            ps += [quantize_piece(p0, p1, cab["radius"], cab["colour"], cab["shade"], arc) for p0, p1 in zip(v[:-1], v[1:])]
            arc += 1
        for cab in d["cables"]:
            v = cab["poly"]
            ps.append(quantize_piece(v[0], v[0], 1.5 * cab["radius"], cab["cap_colour"], cab["shade"], arc))
            arc += 1
        return ps

    def labels(self, d):
        """float32 [K, M, 3] (u, v, flag) of scene description d; empty slots (0, 0, 0).  The
        row of a line class is empty."""
        out = np.zeros((len(self.classes), self.instances, 3), dtype=np.float32)
        for k, c in enumerate(self.classes):
            if c in LINE_CLASSES:
                continue
            p = d["labels"][c]
            out[k, :len(p), :2] = p
            out[k, :len(p), 2] = 1.0
        return out

    def line_labels(self, d):
        """float32 [K, S, 5] (x0, y0, x1, y1, flag) of scene description d, S = cables[1] *
        segments: the "cable" row holds the cables' pieces, vertex pair by vertex pair, in
        cable order then piece order; every other row, and the slots past the last piece,
        are empty (0, 0, 0, 0, 0).  None when no class is a line class."""
        if not self.line_slots:
            return None
        out = np.zeros((len(self.classes), self.line_slots, 5), dtype=np.float32)
        k = self.classes.index("cable")
        at = 0
        for cab in d["cables"]:
            v = cab["poly"]
            out[k, at:at + len(v) - 1, 0:2] = v[:-1]
            out[k, at:at + len(v) - 1, 2:4] = v[1:]
            out[k, at:at + len(v) - 1, 4] = 1.0
            at += len(v) - 1
        return out

    def plan(self, indices, epoch=0, hw=None):
        """The SynthPlan of one batch: scene `indices[b]` of `epoch` for image b."""
        if hw is None:
            raise HkpError("CableScenes.plan: hw=(h, w) is required")
        descs = [self.sample(i, epoch, hw) for i in indices]
        if not descs:
            raise HkpError("CableScenes.plan: no indices")
        return SynthPlan(hw, [self.pieces(d) for d in descs], [d["background"] for d in descs],
                         pts=np.stack([self.labels(d) for d in descs]), fallback=[d["fallback"] for d in descs],
                         descs=descs,
                         lines=np.stack([self.line_labels(d) for d in descs]) if self.line_slots else None)

    def __call__(self, n, hw, index=None, epoch=None):
        """(img uint8 [n,H,W,3] on the current device, pts float32 [n,K,M,3] on it) of n
        scenes: numbered on from the last call under `self.epoch`, unless `index` (one
        per image) and `epoch` are given."""
        from . import ops
        if index is None:
            index = range(self._calls, self._calls + int(n))
            self._calls += int(n)
        plan = self.plan([int(i) for i in index], self.epoch if epoch is None else epoch, hw)
        img = ops.synth_cables_u8(plan)
        return img, torch.from_numpy(plan.pts).to(img.device)


def from_config(cfg, num_keypoints):
    """config.SYNTH -> (train scenes, test scenes, scenes per train epoch, test scenes):
    cfg holds CableScenes's keyword arguments plus "train" and "test" (scene counts) and
    "seed"; the test scenes are drawn under seed + 1.  ValueError for anything else."""
    import inspect
    if not isinstance(cfg, dict):
        raise ValueError("config.SYNTH must be None or a dict, got %r" % (cfg,))
    for k in ("train", "test"):
        if k not in cfg or int(cfg[k]) != cfg[k] or int(cfg[k]) < 1:
            raise ValueError("config.SYNTH needs %r: a scene count of at least 1, got %r" % (k, cfg.get(k)))
    known = set(inspect.signature(CableScenes.__init__).parameters) - {"self"}
    kw = {k: v for k, v in cfg.items() if k not in ("train", "test")}
    if set(kw) - known:
        raise ValueError("config.SYNTH: unknown keys %s (known: train, test, %s)"
                         % (sorted(set(kw) - known), ", ".join(sorted(known))))
    seed = int(kw.pop("seed", 0))
    train, test = CableScenes(seed=seed, **kw), CableScenes(seed=seed + 1, **kw)
    if len(train.classes) != int(num_keypoints):
        raise ValueError("config.SYNTH: NUM_KEYPOINTS = %d but the scenes label %d classes %r"
                         % (num_keypoints, len(train.classes), train.classes))
    return train, test, int(cfg["train"]), int(cfg["test"])
