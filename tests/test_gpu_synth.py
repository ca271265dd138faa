"""hkp_synth_cables_u8 on the GPU: the kernel against its numpy restatement
(tests/_synth_ref.py) bit for bit at every launch path, the sampler's scenes, the
data path (SynthDataset, DeviceBatches), the join with the target / decode / metrics
and with the Trainer, and train.py with config.SYNTH."""
import numpy as np
import pytest
import torch

import _synth_ref as R

pytestmark = pytest.mark.gpu

BGS = [{"bg0": (10, 60, 200), "bg1": (250, 20, 30), "key": (123456789, 4242), "cell_log2": 4},
       {"bg0": (0, 0, 0), "bg1": (255, 255, 255), "key": (7, 0xFFFFFFFF), "cell_log2": 6},
       {"bg0": (90, 90, 90), "bg1": (90, 90, 90), "key": (0, 0), "cell_log2": 12}]


def _ordinary(h, w, seed):
    """One image's geometry that reaches every feature at size h x w: a piece entirely
    outside the picture, pieces across tile borders in both directions, zero-length pieces
    (discs), radius 1 px and 32 px, a self-crossing cable, a second cable crossing it, and
    a cap drawn last.  (polylines, radii, colours, shades)"""
    rng = np.random.default_rng(seed)
    t = np.linspace(0.0, 2.0 * np.pi, 25)
    loop = np.stack([w * (0.5 + 0.45 * np.sin(t)), h * (0.5 + 0.45 * np.sin(2.0 * t))], 1)      # a figure of eight
    polys = [np.array([[w + 40.0, h + 40.0], [w + 90.0, h + 55.0]]),                             # outside
             np.array([[w * 0.3, h * 0.6]]),                                                     # a 32 px disc
             loop,
             np.array([[-3.0, h * 0.2], [w * 0.5, h * 0.55], [w + 2.0, h * 0.9]]),               # crosses the loop
             np.array([[0.5, 0.25], [w - 1.0, 0.25]]),                                           # a 1 px line on row 0
             np.array([[w * 0.7, -2.0], [w * 0.7 + 0.3, h + 2.0]]),                              # top to bottom
             np.array([loop[0]]),                                                                # the cap
             np.array([[w - 1.0, h - 1.0]])]                                                     # 1 px disc in the corner
    radii = [5.0, 32.0, 2.6, 3.3, 1.0, 1.0, 3.9, 1.0]
    cols = [tuple(int(v) for v in rng.integers(0, 256, 3)) for _ in polys]
    shades = [int(v) for v in rng.integers(0, 257, len(polys))]
    return polys, radii, cols, shades


def _plan(hw, images, bgs):
    from hkp.synth import SynthPlan
    return SynthPlan.from_polylines(hw, [im[0] for im in images], [im[1] for im in images], [im[2] for im in images],
                                    background=bgs, shades=[im[3] for im in images])


def _crowd(h, w, seed, n=512):
    """512 short pieces and discs all over (and around) the picture, each its own arc."""
    rng = np.random.default_rng(seed)
    a = rng.uniform((-8, -8), (w + 8, h + 8), (n, 2))
    d = rng.uniform(-14, 14, (n, 2)) * (rng.random((n, 1)) < 0.8)
    polys = [np.stack([p, p + q]) if q.any() else p[None] for p, q in zip(a, d)]
    return (polys, [float(r) for r in rng.uniform(1.0, 6.0, n)],
            [tuple(int(v) for v in c) for c in rng.integers(0, 256, (n, 3))], [int(v) for v in rng.integers(0, 257, n)])


EMPTY = ([], [], [], [])
CASES = {
    "1x3x5 below a tile, bytes": ((3, 5), lambda h, w: [_ordinary(h, w, 1)]),
    "2x16x64 one tile, dwords": ((16, 64), lambda h, w: [_ordinary(h, w, 2), _ordinary(h, w, 3)]),
    "2x17x68 a row and a dword over": ((17, 68), lambda h, w: [_ordinary(h, w, 4), _ordinary(h, w, 5)]),
    "1x33x131 odd width": ((33, 131), lambda h, w: [_ordinary(h, w, 6)]),
    "3x40x200 empty, 512 pieces, ordinary": ((40, 200), lambda h, w: [EMPTY, _crowd(h, w, 7), _ordinary(h, w, 8)]),
}


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_equals_restatement(cuda_device, name):
    from hkp import ops
    (h, w), make = CASES[name]
    images = make(h, w)
    plan = _plan((h, w), images, [BGS[i % 3] for i in range(len(images))])
    assert [sc.seg_cnt for sc in plan.scenes] == [sum(max(len(p) - 1, 1) for p in im[0]) for im in images]
    want = torch.from_numpy(R.render(plan))
    with torch.cuda.device(cuda_device):
        got = ops.synth_cables_u8(plan)
        again = ops.synth_cables_u8(plan)
        pre = torch.full((plan.n, h, w, 3), 77, dtype=torch.uint8, device=cuda_device)
        assert ops.synth_cables_u8(plan, out=pre) is pre
    assert got.dtype == torch.uint8 and tuple(got.shape) == (plan.n, h, w, 3)
    bad = (got.cpu() != want).nonzero()
    assert len(bad) == 0, (len(bad), bad[:5].tolist())
    assert torch.equal(again, got) and torch.equal(pre, got)
    assert want.float().std() > 5                              # a picture, not a constant


def test_byte_path_at_a_width_of_four(cuda_device):
    """An output view one byte off a 4-byte boundary: the byte path at w % 4 == 0; the
    bytes around the view stay as they were."""
    from hkp import ops
    h, w = 17, 68
    plan = _plan((h, w), [_ordinary(h, w, 4), _ordinary(h, w, 5)], BGS[:2])
    want = torch.from_numpy(R.render(plan))
    nbytes = 2 * h * w * 3
    with torch.cuda.device(cuda_device):
        flat = torch.full((nbytes + 8,), 201, dtype=torch.uint8, device=cuda_device)
        view = flat[1:1 + nbytes].view(2, h, w, 3)
        assert view.data_ptr() % 4 == 1
        ops.synth_cables_u8(plan, out=view)
    assert torch.equal(view.cpu(), want)
    assert flat[0].item() == 201 and (flat[1 + nbytes:] == 201).all()
    with pytest.raises(ops.HkpError):
        ops.synth_cables_u8(plan, out=flat[:nbytes].view(2, w, h, 3))


def test_sampler_scenes_equal_restatement(cuda_device):
    from hkp import ops
    from hkp.synth import CableScenes
    plan = CableScenes(seed=3).plan(range(8), 0, (96, 128))
    with torch.cuda.device(cuda_device):
        got = ops.synth_cables_u8(plan)
    assert torch.equal(got.cpu(), torch.from_numpy(R.render(plan)))
    assert plan.pts.shape == (8, 4, 8, 3)


# ------------------------------------------------------------ data path ----
def test_device_batches_and_items(cuda_device):
    from hkp import ops
    from hkp.geometry import GeometricAugmentation
    from hkp.synth import CableScenes
    from src.dataset import DeviceBatches, SynthDataset, transform
    cs, hw = CableScenes(seed=9), (96, 128)
    ds = SynthDataset(cs, 10, hw, device=cuda_device)
    with torch.cuda.device(cuda_device):
        whole = cs.plan(range(10), 0, hw)
        want = ops.synth_cables_u8(whole)
        for bs in (4, 1):
            imgs, pts = zip(*[(i.clone(), p.clone()) for i, p in DeviceBatches(ds, bs, device=cuda_device)])
            assert len(imgs) == (3 if bs == 4 else 10) and imgs[0].dtype == torch.uint8
            assert torch.equal(torch.cat(imgs), want)
            assert torch.equal(torch.cat(pts).cpu(), torch.from_numpy(whole.pts)) and pts[0].dtype == torch.float32
        # the second epoch of one DeviceBatches draws new scenes; a fixed dataset does not
        it = DeviceBatches(ds, 10, device=cuda_device)
        first, second = next(iter(it))[0].clone(), next(iter(it))[0].clone()
        assert torch.equal(first, want) and torch.equal(second, ops.synth_cables_u8(cs.plan(range(10), 1, hw)))
        fx = DeviceBatches(SynthDataset(cs, 10, hw, fixed=True, device=cuda_device), 10, device=cuda_device)
        assert torch.equal(next(iter(fx))[0], want) and torch.equal(next(iter(fx))[0], want)
        # geometric: the picture through the warp, the labels through apply_points
        ga = GeometricAugmentation(seed=2, rotate=(-20, 20), hflip=0.5, keep_inside=False)
        img, pts = next(iter(DeviceBatches(ds, 4, device=cuda_device, geometric=ga)))
        gplan = ga.plan(range(4), 0, uvs=whole.pts[:4], hw=hw)
        assert torch.equal(img, ops.warp_affine_u8(want[:4].contiguous(), gplan))
        assert torch.equal(pts.cpu(), torch.from_numpy(gplan.apply_points(whole.pts[:4])))
        # items
        raw, rpts = ds.raw(6)
        assert np.array_equal(raw, want[6].cpu().numpy()) and torch.equal(rpts.cpu(), torch.from_numpy(whole.pts[6]))
        item, ipts = ds[6]
        assert torch.equal(item, transform(raw)) and torch.equal(ipts, rpts)
        ds.set_epoch(1)
        assert not np.array_equal(ds.raw(6)[0], raw)
        dense = SynthDataset(cs, 10, hw, return_uv=False, device=cuda_device)[6][1]
        assert torch.equal(dense, ops.gauss_target_multi(rpts[None].contiguous(), 96, 128, 8)[0])


# ------------------------------------------------- join with the rest ----
def test_labels_are_in_the_frame_of_target_decode_and_metrics(cuda_device):
    """gauss_target_multi(pts) sampled on the stride-8 lattice as logits -> hkp_heat_peaks
    -> KeypointMetrics: recall 1 at 8 px on every class with instances.  (H - 1, W - 1
    multiples of 8: the lattice nodes are pixels; min_sep 32 keeps two maxima of one plane
    apart on a stride-8 lattice at sigma 8.)"""
    from hkp import ops
    from hkp.metrics import KeypointMetrics
    from hkp.synth import CableScenes
    import _instances_ref as iref
    H, W = 193, 257
    plan = CableScenes(seed=4, min_sep=32.0).plan(range(8), 0, (H, W))
    assert not plan.fallback.any()
    pts = torch.from_numpy(plan.pts).to(cuda_device)
    with torch.cuda.device(cuda_device):
        target = ops.gauss_target_multi(pts, H, W, 8.0).cpu().numpy()
        low = torch.from_numpy(iref.lowres_logits(target)).to(cuda_device)
        peaks, counts = ops.heat_peaks(low, H, W, max_peaks=8, radius=1, threshold=0.5)
        m = KeypointMetrics(4, (8.0,), device=cuda_device)
        m.update(peaks, counts, pts)
    res = m.compute()
    inst = [r["instances"] for r in res["per_class"]]
    print("instances per class:", inst, "mean error px:", [r["mean_error_px"] for r in res["per_class"]])
    assert inst == [int(v) for v in plan.pts[:, :, :, 2].sum((0, 2))] and min(inst) > 0
    for r in res["per_class"]:
        assert r["recall"] == [1.0], r
    assert any(r["absent_planes"] > 0 for r in res["per_class"])          # some picture has no crossing / blob


def test_training_lowers_the_held_out_loss(cuda_device):
    """R18-8s, 96x128, B = 4, one cable, classes (cap, tail): STEPS Trainer steps on fresh
    scenes; the BCE of 16 fixed held-out scenes must be lower afterwards (a sign condition;
    what recall training reaches is tools/synth_train.py's record, not asserted)."""
    from hkp import autograd as hkp_autograd
    from hkp import train
    from hkp.synth import CableScenes
    from oracle import recipe
    from src.dataset import DeviceBatches, SynthDataset
    from src.model import KeypointsGauss
    STEPS, hw = 24, (96, 128)
    kw = dict(classes=("cap", "tail"), cables=(1, 1), blobs=(0, 2), instances=2)
    model = KeypointsGauss(2, hw[0], hw[1], backbone="resnet18", pretrained=False)
    model.load_state_dict(recipe.seeded_state_dict("resnet18", 23))
    model = model.to(cuda_device)
    with torch.cuda.device(cuda_device):
        held = next(iter(DeviceBatches(SynthDataset(CableScenes(seed=11, **kw), 16, hw, fixed=True, device=cuda_device),
                                       16, device=cuda_device)))

        def held_out():
            with torch.no_grad():
                return hkp_autograd.heatmap_loss(model(held[0]), pts=held[1], sigma=8.0, kind="bce", absent="zero").item()

        before = held_out()
        tr = train.Trainer(model, loss="bce", absent="zero")
        last = None
        for img, pts in DeviceBatches(SynthDataset(CableScenes(seed=10, **kw), 4 * STEPS, hw, device=cuda_device), 4,
                                      device=cuda_device):
            last = tr.step(img, pts=pts)
        after = held_out()
    print("held-out BCE before %.6f after %.6f; last train loss %.6f" % (before, after, last.item()))
    assert np.isfinite(after) and after < before


def test_train_py_runs_on_scenes_alone(tmp_path, monkeypatch, capsys, cuda_device):
    import train as train_mod
    monkeypatch.chdir(tmp_path)                                            # no data/ directory here
    for name, v in (("IMG_HEIGHT", 96), ("IMG_WIDTH", 128), ("NUM_KEYPOINTS", 2), ("batch_size", 4), ("epochs", 1),
                    ("BACKBONE", "resnet18"),
                    ("SYNTH", {"train": 8, "test": 4, "seed": 5, "classes": ("cap", "tail"), "instances": 2,
                               "cables": (1, 1)})):
        monkeypatch.setattr(train_mod, name, v)
    torch.manual_seed(5)
    with pytest.warns(UserWarning, match="pretrained"):
        train_mod.main("scenes")
    out = capsys.readouterr().out
    assert "[1,     2] loss:" in out
    train_loss = float(out.split("train loss:")[1].split()[0])
    test_loss = float(out.split("test loss:")[1].split()[0])
    assert np.isfinite(train_loss) and train_loss > 0 and np.isfinite(test_loss) and test_loss > 0
    assert (tmp_path / "checkpoints" / "scenes" / "model_2_1_0.pth").exists()
    assert not (tmp_path / "data").exists()
