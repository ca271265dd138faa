"""CPU checks of the procedural cable scenes (hkp/synth.py): the sampler and its labels,
the fixed-point records, the numpy restatement (tests/_synth_ref.py) against float64
geometry, the dataset layer and the host-side validation of hkp_synth_cables_u8."""
import ctypes
import math

import numpy as np
import pytest

import _synth_ref as R

HW = (480, 640)


@pytest.fixture(scope="module")
def scenes200():
    """Scenes 0..199 of seed 0, default settings, 480x640 (shared, not modified)."""
    from hkp.synth import CableScenes
    cs = CableScenes(seed=0)
    return cs, [cs.sample(i, 0, HW) for i in range(200)]


# ------------------------------------------------------------ sampler ----
def _same(a, b):
    return (a["try"] == b["try"] and len(a["cables"]) == len(b["cables"]) and len(a["blobs"]) == len(b["blobs"])
            and all(np.array_equal(x["poly"], y["poly"]) for x, y in zip(a["cables"], b["cables"]))
            and a["background"] == b["background"])


def test_scene_is_a_function_of_seed_epoch_index():
    from hkp.synth import CableScenes
    cs = CableScenes(seed=5)
    hw = (96, 128)
    whole = cs.plan([7, 3, 11, 4], 2, hw)
    for b, i in enumerate([7, 3, 11, 4]):
        one = cs.plan([i], 2, hw)
        sc, so = whole.scenes[b], one.scenes[0]
        assert sc.seg_cnt == so.seg_cnt
        assert np.array_equal(whole.seg_bytes()[sc.seg_off:sc.seg_off + sc.seg_cnt], one.seg_bytes()[:so.seg_cnt])
        assert bytes(whole.scene_bytes()[b][8:]) == bytes(one.scene_bytes()[0][8:])     # all but the offsets
        assert np.array_equal(whole.pts[b], one.pts[0])
        assert _same(cs.sample(i, 2, hw), CableScenes(seed=5).sample(i, 2, hw))
    assert not _same(cs.sample(7, 2, hw), cs.sample(7, 3, hw))
    assert not _same(cs.sample(7, 2, hw), cs.sample(8, 2, hw))
    assert not _same(cs.sample(7, 2, hw), CableScenes(seed=6).sample(7, 2, hw))


def test_labels_are_the_scene(scenes200):
    cs, ds = scenes200
    for d in ds[:60]:
        pts = cs.labels(d)
        assert pts.shape == (4, 8, 3) and pts.dtype == np.float32
        polys = [c["poly"] for c in d["cables"]]
        ncab = len(polys)
        for k, end in ((0, 0), (1, -1)):                      # cap: vertex 0, tail: the last vertex
            assert pts[k, :, 2].sum() == ncab
            for c, p in enumerate(polys):
                assert np.array_equal(pts[k, c, :2], p[end].astype(np.float32))
        brute = R.brute_crossings(polys)
        on = pts[2, :, 2] > 0
        assert on.sum() == len(brute) == len(d["labels"]["crossing"])
        for x in d["labels"]["crossing"]:
            near = sorted(R.dist_to_polyline(x, p) for p in polys)
            assert near[0] < 1e-9
            # both strands pass through it: two distinct pieces within 1e-9
            hits = sum(R.dist_point_segment(x, p[i], p[i + 1]) < 1e-9 for p in polys for i in range(len(p) - 1))
            assert hits >= 2
        assert pts[3, :, 2].sum() == len(d["blobs"])
        for j, b in enumerate(d["blobs"]):
            assert np.array_equal(pts[3, j, :2], b["centre"].astype(np.float32))
        assert not pts[pts[..., 2] == 0].any()                # empty slots are (0, 0, 0)


def test_every_rule_holds_for_accepted_scenes(scenes200):
    cs, ds = scenes200
    checked = 0
    for d in ds[:80]:
        if d["fallback"]:
            continue
        checked += 1
        lab = d["labels"]
        polys = [c["poly"] for c in d["cables"]]
        m = cs.margin
        for c in ("cap", "tail", "crossing", "blob"):
            p = lab[c]
            assert len(p) <= cs.instances
            for i in range(len(p)):
                assert m - 1e-9 <= p[i][0] <= HW[1] - 1 - m + 1e-9 and m - 1e-9 <= p[i][1] <= HW[0] - 1 - m + 1e-9
                for j in range(i + 1, len(p)):
                    assert math.hypot(*(p[i] - p[j])) >= cs.min_sep
        for p in polys:                                       # a cable never leaves the margin box
            assert p[:, 0].min() >= m - 1e-9 and p[:, 0].max() <= HW[1] - 1 - m + 1e-9
            assert p[:, 1].min() >= m - 1e-9 and p[:, 1].max() <= HW[0] - 1 - m + 1e-9
        assert all(a >= cs.min_angle for _, a in R.brute_crossings(polys))
        for ci, cab in enumerate(d["cables"]):
            poly, r = cab["poly"], cab["radius"]
            n = len(poly) - 1
            for end in (0, n):
                step = 1 if end == 0 else -1
                k = end
                while 0 <= k <= n and math.hypot(*(poly[k] - poly[end])) <= 2 * r + 2:
                    k += step                                 # the end's own neighbourhood
                for cj, other in enumerate(d["cables"]):
                    first, last = 0, None
                    if cj == ci:
                        first, last = (min(k, n), n) if end == 0 else (0, max(k, 0))
                    assert R.dist_to_polyline(poly[end], other["poly"], first, last) >= r + other["radius"] + 2
        for b in d["blobs"]:
            for cab in d["cables"]:
                assert R.dist_to_polyline(b["centre"], cab["poly"]) >= b["radius"] + cab["radius"]
    assert checked >= 60


def test_fallback_scene_and_share(scenes200):
    from hkp.synth import CableScenes
    cs, ds = scenes200
    share = sum(d["fallback"] for d in ds) / len(ds)
    print("fallback share over 200 scenes: %.3f" % share)
    assert share <= 0.05
    tight = CableScenes(seed=0, min_sep=1e6, cables=(2, 2), tries=2)      # no candidate can pass
    plan = tight.plan([0, 1], 0, (96, 128))
    assert plan.fallback.all()
    d = plan.descs[0]
    assert d["try"] == 2 and len(d["cables"]) == 1 and not d["blobs"]
    m = tight.margin
    assert np.allclose(d["cables"][0]["poly"][0], (m, m)) and np.allclose(d["cables"][0]["poly"][-1], (127 - m, 95 - m))
    assert plan.pts[:, :, :, 2].sum(2).tolist() == [[1, 1, 0, 0]] * 2          # one cap, one tail, nothing else
    assert not CableScenes(seed=0).plan([0, 1], 0, HW).fallback.any()


def test_classes_reorder_and_drop_planes():
    from hkp.synth import CableScenes
    full = CableScenes(seed=2).plan([0, 1, 2, 3], 0, (200, 300))
    part = CableScenes(seed=2, classes=("blob", "cap")).plan([0, 1, 2, 3], 0, (200, 300))
    assert part.pts.shape == (4, 2, 8, 3)
    assert np.array_equal(part.pts[:, 0], full.pts[:, 3]) and np.array_equal(part.pts[:, 1], full.pts[:, 0])
    assert np.array_equal(part.seg_bytes(), full.seg_bytes())                 # the picture does not change
    with pytest.raises(ValueError):
        CableScenes(classes=("cap", "knot"))
    with pytest.raises(ValueError):
        CableScenes(instances=17)
    with pytest.raises(ValueError):
        CableScenes(cables=(1, 8), segments=80)                               # more than 512 pieces


# -------------------------------------------------------- fixed point ----
def test_fixed_point_records(scenes200):
    from hkp.synth import quantize_piece
    cs, ds = scenes200
    plan = cs.plan(range(6), 0, HW)
    for i in range(sum(sc.seg_cnt for sc in plan.scenes)):
        s = plan.segs[i]
        assert abs(math.hypot(s.ux, s.uy) / 16384.0 - 1.0) < 2.0 ** -13
        assert s.r_in2 == (s.r - 8) ** 2 and s.r_out2 == (s.r + 8) ** 2 and s.r2 == s.r ** 2
        assert s.inv == (1 << 32) // (s.r_out2 - s.r_in2) and s.inv_r2 == (1 << 32) // s.r2
    for radius in (1.0, 4.3, 8.0, 32.0):
        p = quantize_piece((3.0, 4.0), (40.0, 9.0), radius, (1, 2, 3), 100, 0)
        s = type("S", (), p)
        d2 = np.arange(0, p["r_out2"] + 50, dtype=np.int64)
        a = R.alpha_of_d2(s, d2)
        assert np.all(np.diff(a) <= 0)                                        # monotone
        assert a[0] == 256 and np.all(a[:p["r_in2"] + 1] == 256) and np.all(a[p["r_out2"]:] == 0)
        assert a[p["r_in2"] + 1] >= 254 and a[p["r_out2"] - 1] <= 1 and a.min() == 0 and a.max() == 256
        # the products that are taken in 32 bits fit, the one that does not is the header's
        assert (p["r_out2"] - p["r_in2"] - 1) * p["inv"] < 1 << 32
        assert p["r2"] * p["inv_r2"] <= 1 << 32
    with pytest.raises(RuntimeError):
        quantize_piece((0, 0), (1, 1), 0.4, (1, 2, 3), 0, 0)


# ------------------------------------- restatement against float64 ----
def test_restatement_covers_a_fat_cable_exactly():
    from hkp.synth import SynthPlan
    hw, r, col = (56, 96), 9.0, (30, 200, 90)
    a, b = np.array([10.3, 12.7]), np.array([80.2, 40.1])
    img = R.render(SynthPlan.from_polylines(hw, [[np.stack([a, b])]], [[r]], [[col]], shades=[[0]]))[0]
    bg = R.render(SynthPlan.from_polylines(hw, [[]], [[]], [[]]))[0]
    inside = outside = 0
    for y in range(hw[0]):
        for x in range(hw[1]):
            d = R.dist_point_segment((x, y), a, b)
            if d <= r - 1:
                assert tuple(img[y, x]) == col, (x, y, d)
                inside += 1
            elif d >= r + 1:
                assert np.array_equal(img[y, x], bg[y, x]), (x, y, d)
                outside += 1
    assert inside > 800 and outside > 2000
    assert bg.std() > 1 and 40 <= bg.min() and bg.max() <= 96                # noise between the two colours


def test_restatement_puts_the_later_cable_on_top():
    from hkp.synth import SynthPlan
    hw = (64, 64)
    c0, c1 = (250, 20, 20), (20, 20, 250)
    l0 = np.array([[6.0, 32.0], [58.0, 32.0]])
    l1 = np.array([[32.0, 6.0], [32.0, 58.0]])
    img = R.render(SynthPlan.from_polylines(hw, [[l0, l1], [l1, l0]], [[5.0, 5.0]] * 2, [[c0, c1], [c1, c0]],
                                            shades=[[0, 0]] * 2))
    assert tuple(img[0, 32, 32]) == c1 and tuple(img[1, 32, 32]) == c0
    assert tuple(img[0, 32, 12]) == c0 and tuple(img[0, 12, 32]) == c1      # away from the crossing
    # shading darkens towards the rim and leaves the centreline as it is
    sh = R.render(SynthPlan.from_polylines(hw, [[l0]], [[5.0]], [[c0]], shades=[[200]]))[0]
    assert tuple(sh[32, 20]) == c0 and sh[28, 20, 0] < sh[30, 20, 0] < 250


# ----------------------------------------------------- layers and ABI ----
def test_synth_dataset_indexing():
    from hkp.synth import CableScenes
    from src.dataset import DeviceBatches, SynthDataset
    cs = CableScenes(seed=1, classes=("cap", "tail"), instances=3)
    ds = SynthDataset(cs, 10, (96, 128))
    assert (len(ds), ds.img_height, ds.img_width, ds.num_keypoints, ds.instances) == (10, 96, 128, 2, 3)
    shards = [SynthDataset(cs, 10, (96, 128), rank=r, world=3) for r in range(3)]
    assert [len(s) for s in shards] == [4, 3, 3]
    assert sorted(s.scene_index(i) for s in shards for i in range(len(s))) == list(range(10))
    assert np.array_equal(shards[1].plan([2]).pts, cs.plan([7], 0, (96, 128)).pts)
    with pytest.raises(IndexError):
        shards[1].scene_index(3)
    ds.set_epoch(4)
    assert np.array_equal(ds.plan([5]).seg_bytes(), cs.plan([5], 4, (96, 128)).seg_bytes())
    assert not np.array_equal(ds.plan([5]).pts, cs.plan([5], 0, (96, 128)).pts)
    fixed = SynthDataset(cs, 10, (96, 128), fixed=True)
    fixed.set_epoch(4)
    assert np.array_equal(fixed.plan([5], epoch=9).pts, cs.plan([5], 0, (96, 128)).pts)
    with pytest.raises(ValueError):
        SynthDataset(cs, 10, (96, 128), rank=3, world=3)
    from hkp.resample import Resize
    with pytest.raises(ValueError, match="SynthDataset"):
        DeviceBatches(ds, 4, resize=Resize())
    with pytest.raises(ValueError, match="SynthDataset"):
        DeviceBatches(ds, 4, decode="device")


def test_config_synth_validation():
    import config
    from hkp.synth import from_config
    assert config.SYNTH is None
    tr, te, ntr, nte = from_config({"train": 12, "test": 5, "seed": 3, "classes": ("cap", "tail"), "instances": 2}, 2)
    assert (tr.seed, te.seed, ntr, nte, tr.instances, te.classes) == (3, 4, 12, 5, 2, ("cap", "tail"))
    with pytest.raises(ValueError, match="NUM_KEYPOINTS"):
        from_config({"train": 12, "test": 5}, 2)                              # four classes by default
    with pytest.raises(ValueError, match="'test'"):
        from_config({"train": 12}, 4)
    with pytest.raises(ValueError, match="'train'"):
        from_config({"train": 0, "test": 5}, 4)
    with pytest.raises(ValueError, match="unknown keys"):
        from_config({"train": 1, "test": 1, "knots": 3}, 4)
    with pytest.raises(ValueError, match="dict"):
        from_config(True, 4)


def _abi_call(plan, n=None, h=None, w=None, nsegs=None):
    from hkp import _lib
    p = ctypes.c_void_p(16)                                                  # never dereferenced: validation fails first
    return _lib.call("hkp_synth_cables_u8", plan.n if n is None else n, plan.hw[0] if h is None else h,
                     plan.hw[1] if w is None else w, p, plan.scenes, p, plan.segs, p,
                     plan.nsegs if nsegs is None else nsegs, None)


def test_abi_rejects_bad_records_on_the_host():
    from hkp import _lib
    from hkp.synth import SynthPlan

    def plan(npieces=3):
        line = np.array([[2.0, 2.0], [20.0, 9.0]])
        return SynthPlan.from_polylines((32, 40), [[line] * npieces], [[3.0] * npieces], [[(1, 2, 3)] * npieces])

    assert ctypes.sizeof(_lib.SynthSeg) == 64 and ctypes.sizeof(_lib.SynthScene) == 64
    with pytest.raises(_lib.HkpError, match="outside 1..4096"):
        _abi_call(plan(), w=0)
    with pytest.raises(_lib.HkpError, match="outside 1..4096"):
        _abi_call(plan(), h=4097)
    p = plan(512)
    p.scenes[0].seg_cnt = 513
    with pytest.raises(_lib.HkpError, match="513 pieces"):
        _abi_call(p, nsegs=600)
    for r in (0, 33 * 16):
        p = plan()
        p.segs[1].r = r
        with pytest.raises(_lib.HkpError, match="radius"):
            _abi_call(p)
    p = plan()
    p.segs[2].inv += 1                                                        # constants that do not belong to r
    with pytest.raises(_lib.HkpError, match="do not belong"):
        _abi_call(p)
    p = plan()
    with pytest.raises(_lib.HkpError, match="run past the table"):
        _abi_call(p, nsegs=2)
    p.scenes[0].seg_off = 1
    with pytest.raises(_lib.HkpError, match="run past the table"):
        _abi_call(p)
    p = plan()
    p.scenes[0].cell_log2 = 3
    with pytest.raises(_lib.HkpError, match="cell_log2"):
        _abi_call(p)
    p = plan()
    p.segs[0].x0 = (1 << 17) + 1
    with pytest.raises(_lib.HkpError, match="vertex"):
        _abi_call(p)
    with pytest.raises(_lib.HkpError, match="at most 512|512"):
        plan(513)
