#!/usr/bin/env python3
"""The bits of the heatmap losses: runs gauss_target_multi, heat_loss, heat_loss_multi (with
its quality focal kind and its instances divisor) and heat_loss_planes through hkp.ops on the
GPU, on the seeded inputs of tests/test_gpu_instances.py and tests/test_gpu_planes.py, and
writes the SHA-256 of every output's bytes (loss, dheat, plane_loss, plane_used) as JSON.

tests/golden/loss_bits_parent.json is this tool's output on the library of the commit before
the loss kernels were folded into one body; tests/test_gpu_loss_bits.py recomputes every case
on the current tree and requires every hash to match.  With -ffp-contract=off and no fast-math
the compiler may not reorder the sums, so a mismatch under the same compiler means that an
operation order changed.  After a compiler upgrade regenerate the file, knowingly:

    python tools/loss_bits.py --out tests/golden/loss_bits_parent.json

`--lib PATH` runs another build of the library (the same C ABI); `--commit` names the commit
it was built from (default: this checkout's HEAD)."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(REPO, "tests"), os.path.join(REPO, "hulk-keypoints_amd"), REPO):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

ABSENT = ("zero", "ignore")
KINDS = (("bce", 2.0), ("mse", 2.0), ("qfl", 2.0), ("qfl", 1.5))
OUTPUTS = ("loss", "dheat", "plane_loss", "plane_used")
GROUPS = ("target", "heat_loss", "multi", "ex", "planes", "topk", "unaligned")


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _outputs(out):
    return {name: _sha(t) for name, t in zip(OUTPUTS, out) if t is not None}


def compiler_line():
    """The `HIP version` line of the hipcc that builds the library here."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    try:
        text = subprocess.run([hipcc, "--version"], capture_output=True, text=True, check=True).stdout
    except (OSError, subprocess.CalledProcessError) as e:
        return "unknown (%s)" % e
    lines = [ln.strip() for ln in text.splitlines() if ln.strip()]
    return next((ln for ln in lines if ln.startswith("HIP version")), lines[0] if lines else "unknown")


def _off_by_4_bytes(p):
    """p's values in a contiguous tensor that starts 4 bytes off a 16-byte boundary."""
    buf = torch.empty(p.numel() + 1, device=p.device)
    off = buf[1:].view(p.shape)
    off.copy_(p)
    assert off.is_contiguous() and off.data_ptr() % 16 == 4
    return off


def _nonpositive(w):
    """Weights with a 0, a negative one and a NaN (tests/test_gpu_planes.py::test_unlabelled_planes),
    as many of them as leave one plane labelled."""
    w = w.clone()
    n, k = w.shape
    for i, v in zip((1, k, n * k - 1), (0.0, -1.0, float("nan"))):
        if i < n * k and int((w > 0).sum()) > 1:
            w.view(-1)[i] = v
    return w


def compute(dev, group=None):
    """{case: {output: sha256}} of every case, or of one group's; the inputs' own hash is the
    case "inputs" of every group."""
    from hkp import ops
    from test_gpu_focal import _labels
    from test_gpu_instances import SHAPES, _heat, _points
    from test_gpu_planes import TOPK_SHAPES, _weights
    want = lambda g: group is None or group == g       # noqa: E731
    cases = {}
    seen = hashlib.sha256()
    for shape in SHAPES + TOPK_SHAPES[:3]:
        topk_only = shape not in SHAPES
        n, k, m, H, W = shape
        p = _heat(shape, seed=4)
        w = _weights(shape)
        labels = {a: _labels(shape, a) for a in ABSENT}
        for t in (p, w, labels["zero"], labels["ignore"]):
            seen.update(t.numpy().tobytes())
        pd, wd = p.to(dev), w.to(dev)
        if not topk_only and want("target"):
            for sigma in (8.0, 0.75):
                out = ops.gauss_target_multi(_points(shape).to(dev), H, W, sigma)
                cases["target %s sigma %g" % (shape, sigma)] = {"target": _sha(out)}
        if not topk_only and want("heat_loss"):
            uv = torch.nan_to_num(_points(shape)[:, :, 0, :2], nan=3.5, posinf=1.0).contiguous().to(dev)
            dense = ops.gauss_target(uv, H, W, 8.0)
            for kind in ("bce", "mse"):
                for grad in (True, False):
                    tag = "heat_loss %s %s grad %d" % (shape, kind, grad)
                    cases[tag + " uv"] = _outputs(ops.heat_loss(pd, uv=uv, kind=kind, want_grad=grad))
                    cases[tag + " dense"] = _outputs(ops.heat_loss(pd, target=dense, kind=kind, want_grad=grad))
        for absent in ABSENT:
            ptsd = labels[absent].to(dev)
            if not topk_only and want("multi"):
                for kind in ("bce", "mse"):
                    for grad in (True, False):
                        cases["multi %s %s %s grad %d" % (shape, absent, kind, grad)] = _outputs(
                            ops.heat_loss_multi(pd, ptsd, 8.0, kind, absent, grad))
            if not topk_only and want("ex"):
                forms = [("qfl", 2.0, "elements", True), ("qfl", 1.5, "elements", True)]
                forms += [(kind, beta, "instances", True) for kind, beta in KINDS]
                forms += [("qfl", 1.5, "instances", False)]
                for kind, beta, norm, grad in forms:
                    cases["ex %s %s %s %g %s grad %d" % (shape, absent, kind, beta, norm, grad)] = _outputs(
                        ops.heat_loss_multi(pd, ptsd, 8.0, kind, absent, grad, beta=beta, norm=norm))
            if not topk_only and want("planes"):
                forms = (("none", None, "elements", True), ("none", None, "elements", False),
                         ("weights", wd, "elements", True), ("weights", wd, "instances", True),
                         ("nonpositive", _nonpositive(w).to(dev), "elements", True))
                for kind, beta in KINDS:
                    for name, ww, norm, grad in forms:
                        cases["planes %s %s %s %g %s %s grad %d" % (shape, absent, kind, beta, name, norm, grad)] = \
                            _outputs(ops.heat_loss_planes(pd, ptsd, 8.0, kind, absent, grad, beta=beta, norm=norm,
                                                          weights=ww))
            if (topk_only or shape in (SHAPES[0], SHAPES[3], SHAPES[5])) and want("topk"):
                for kind, beta in KINDS:
                    for name, ww, grad in (("none", None, True), ("weights", wd, True), ("weights", wd, False)):
                        cases["topk2 %s %s %s %g %s grad %d" % (shape, absent, kind, beta, name, grad)] = _outputs(
                            ops.heat_loss_planes(pd, ptsd, 8.0, kind, absent, grad, beta=beta, weights=ww, topk=2))
            if shape == SHAPES[4] and want("unaligned"):
                # W % 4 == 0 from a base 4 bytes off: the scalar path
                off = _off_by_4_bytes(pd)
                tag = "unaligned %s %s " % (shape, absent)
                cases[tag + "multi bce"] = _outputs(ops.heat_loss_multi(off, ptsd, 8.0, "bce", absent))
                cases[tag + "ex qfl 1.5"] = _outputs(ops.heat_loss_multi(off, ptsd, 8.0, "qfl", absent, beta=1.5))
                cases[tag + "planes weights"] = _outputs(ops.heat_loss_planes(off, ptsd, 8.0, "bce", absent, weights=wd))
                cases[tag + "topk2"] = _outputs(ops.heat_loss_planes(off, ptsd, 8.0, "qfl", absent, weights=wd, topk=2))
    cases["inputs"] = {"sha256": seen.hexdigest()}
    return cases


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--lib", help="another build of libhulkkp.so to run in place of the tree's")
    ap.add_argument("--commit", help="the commit the library was built from (default: HEAD)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("loss_bits: no GPU (the kernels are what is recorded)")
    from hkp import _lib
    if args.lib:
        _lib.use_library(os.path.abspath(args.lib))
    commit = args.commit
    if commit is None:
        r = subprocess.run(["git", "-C", REPO, "rev-parse", "HEAD"], capture_output=True, text=True)
        commit = r.stdout.strip() if r.returncode == 0 else "unknown"
    cases = compute(torch.device("cuda", 0))
    doc = {"tool": "loss_bits", "compiler": compiler_line(), "torch": torch.__version__, "commit": commit,
           "device": torch.cuda.get_device_name(0), "cases": cases}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print("loss_bits: %d cases, %d hashes -> %s" % (len(cases), sum(len(c) for c in cases.values()), args.out))


if __name__ == "__main__":
    main()
