"""The f16x3 / plain-fp16 conv launcher starts the kernels it started before it read its
launches from the plan of csrc/x3_plan.h: tests/golden/x3_launch_bits.json holds the SHA-256
of the output bytes (and of the BN partials, where the launch writes them) of a short seeded
list that reaches every kernel id and launch form the plan can emit, recorded with the library
of the commit named in the file (`python tests/test_gpu_x3_launch_bits.py out.json <commit>`, twice:
the two files were identical).  A kernel id wired to the wrong body passes every tolerance
test; it cannot pass this one.

The plan depends on the CU count, so the fixture names the count it was recorded on and the
test fails (it does not skip) on a device with another."""
import hashlib
import json
import os
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "hulk-keypoints_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(REPO, "tests", "golden", "x3_launch_bits.json")

SMALL = (1, 9, 11, 256, 256, 3, 2, 1, 1)            # one partial m-tile (30 rows)
HALO = (1, 32, 64, 64, 64, 3, 1, 1, 1)              # 8 256-row m-tiles of 8x32 patches
ROUND1 = (1, 240, 320, 256, 256, 1, 1, 0, 1)        # M = 76,800: 300 m-tiles, one round of 256 CUs + 44
ROUND1_64 = (1, 240, 320, 64, 256, 1, 1, 0, 1)      # the same rows, two K-steps
PART = (1, 120, 160, 256, 256, 1, 1, 0, 1)          # M = 19,200: 75 m-tiles, less than a round
STEM = (1, 16, 64, 3, 64, 7, 2, 3, 1)               # 8 x 32 outputs: one patch
STEM_ODD = (1, 18, 70, 3, 64, 7, 2, 3, 1)           # 9 x 35 outputs: no whole patch

# (case, entry, (n, h, w, cin, cout, k, stride, pad, dil), HKP_TILE_* policy, stream-K workspace,
#  the kernels it starts on 256 CUs)
CASES = [
    # the six conv_x3_kernel forms
    ("tile256", "x3", SMALL, 3, True, ["conv_x3_kernel<256, false, false, 16, false, 3>"]),
    ("tile128mf16", "x3", SMALL, 4, True, ["conv_x3_kernel<128, false, false, 16, false, 3>"]),
    ("tile128mf32", "x3", SMALL, 5, True, ["conv_x3_kernel<128, false, false, 32, false, 3>"]),
    ("pair64", "x3", SMALL, 6, True, ["conv_x3_kernel<64, false, true, 16, false, 3>"]),
    ("sk128", "x3", (1, 20, 30, 64, 128, 1, 1, 0, 1), 2, True, ["conv_x3_kernel<128, false, false, 16, true, 3>"]),
    ("sk64", "x3", (1, 20, 30, 64, 64, 1, 1, 0, 1), 2, True, ["conv_x3_kernel<64, false, false, 32, true, 3>"]),
    ("pair64_w16", "w16", SMALL, 6, True, ["conv_x3_kernel<64, false, true, 16, false, 2>"]),
    ("a3_nows", "x3", ROUND1, 11, False, ["conv_x3_a3_kernel<3>"]),
    # A3: alone (a3_nows above), with the in-launch tail, the tail-only grid; the two-launch tail
    ("a3", "x3", SMALL, 11, True, ["conv_x3_a3_kernel<3>"]),
    ("a3_tail", "x3", ROUND1, 11, True, ["conv_x3_a3_kernel<3>"]),
    ("a3_tail_only", "x3", PART, 11, True, ["conv_x3_a3_kernel<3>"]),
    ("a3_f16", "f16", ROUND1, 11, True, ["conv_x3_a3_kernel<1>"]),
    ("tail2", "x3", ROUND1, 9, True, ["conv_x3_kernel<256, false, false, 16, false, 3>", "conv_x3_tail_kernel<256, 3>"]),
    ("tail_only", "x3", PART, 9, True, ["conv_x3_kernel<256, false, false, 16, false, 3>", "conv_x3_tail_kernel<256, 3>"]),
    # the shorter A3 tiles and the mixed-height launch (three regions, two regions)
    ("a3_192", "x3", SMALL, 15, True, ["conv_x3_a3_192_kernel<3>"]),
    ("a3_160", "x3", SMALL, 16, True, ["conv_x3_a3_160_kernel<3>"]),
    ("a3_160x128", "x3", (3, 37, 41, 128, 128, 1, 1, 0, 1), 16, True, ["conv_x3_a3_160x128_kernel<3>"]),
    ("mix3", "x3", (2, 240, 320, 64, 256, 1, 1, 0, 1), 17, True, ["conv_x3_a3_mix_kernel<3>"]),
    ("mix2", "x3", (1, 256, 448, 64, 256, 1, 1, 0, 1), 17, True, ["conv_x3_a3_mix_kernel<3>"]),
    # halo, and halo with the fused input BN
    ("halo_x3", "x3", HALO, 0, True, ["conv_x3_halo_kernel<3>"]),
    ("halo_f16", "f16", HALO, 0, True, ["conv_x3_halo_kernel<1>"]),
    ("halo_bnin_x3", "x3_bnin", HALO, 0, True, ["conv_x3_halo_bnin_kernel<3>"]),
    ("halo_bnin_f16", "f16_bnin", HALO, 0, True, ["conv_x3_halo_bnin_kernel<1>"]),
    # DUO: at most two blocks per CU (no stagger), and more
    ("duo_small", "f16", SMALL, 13, True, ["conv_x3_duo_kernel<1>"]),
    ("duo_large", "f16", ROUND1_64, 13, True, ["conv_x3_duo_kernel<1>"]),
    # dgrads, the fused-BN fp16 epilogue, the stem
    ("dgrad", "dgrad", (2, 11, 13, 64, 256, 3, 1, 1, 1), 0, True, None),
    ("dgrad_halo", "dgrad", HALO, 0, True, ["conv_x3_halo_kernel<3>"]),
    ("dgrad_s2", "dgrad_s2", (1, 18, 22, 64, 64, 3, 2, 1, 1), 0, True, None),
    ("f16bn", "f16bn", HALO, 0, True, None),
    ("stem_planes", "stem_planes", STEM, 0, True, ["conv_x3_stem_patch_kernel<0>"]),
    ("stem_image", "stem_image", STEM, 0, True, ["conv_x3_stem_patch_kernel<1>"]),
    ("stem_u8", "stem_u8", STEM, 0, True, ["conv_x3_stem_patch_kernel<2>"]),
    ("stem_pair", "stem_planes", STEM_ODD, 0, True, ["conv_x3_kernel<64, true, true, 16, false, 3>"]),
]

# the launch forms a kernel id alone does not tell apart: (case, what its first launch must say)
FORMS = {
    "a3": dict(main_blocks=0, tail_groups=8, blocks=8),        # one m-tile as eight K segments
    "tail_only": dict(blocks=0),                               # no full round: only the tail kernel starts
    "a3_tail": dict(main_blocks=256, tail_groups=88, tail_mt0=256),
    "a3_tail_only": dict(main_blocks=0, tail_groups=150, tail_mt0=0),
    "a3_nows": dict(main_blocks=0, tail_groups=0, blocks=300, uses_ws=0),
    "mix3": dict(mix_b1=256, mix_b2=512),
    "duo_small": dict(stagger_ns=0),
    "sk128": dict(uses_ws=1),
}


def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def run_case(dev, entry, shape, tile, sk):
    """The hashes {output name: sha256} of one seeded launch."""
    from hkp import ops
    n, h, w, cin, cout, k, st, pad, dil = shape
    if entry.startswith("stem"):
        wp = ops.stem_weight_pack_x3((_rand(cout, cin, 7, 7, seed=3) * 0.1).to(dev))
        if entry == "stem_u8":
            x = torch.randint(0, 256, (n, h, w, cin), generator=torch.Generator().manual_seed(4), dtype=torch.uint8).to(dev)
        else:
            x = _rand(n, cin, h, w, seed=4).to(dev)
        y, part = ops.conv2d_fwd_stem_x3(x, wp, cout, tile=tile, image_direct=entry != "stem_planes")
        return {"y": _sha(y), "part": _sha(part)}
    x = torch.relu(_rand(n, h, w, cin, seed=1)).to(dev)
    wt = (_rand(cout, k, k, cin, seed=2) * (2.0 / (k * k * cout)) ** 0.5).to(dev)
    ident = torch.cat([torch.ones(cin), torch.zeros(cin)]).to(dev)
    ho, wo = ops.conv_out_hw(h, w, k, k, st, pad, dil)
    if entry in ("x3", "w16"):
        xs = ops.bn_apply(x, ident, relu=False, split=3, keep_fp32=False)
        y, part = ops.conv2d_fwd_x3(xs, ops.weight_pack_x3(wt), st, pad, dil, sk=sk, tile=tile,
                                    products=2 if entry == "w16" else 3)
        return {"y": _sha(y), "part": _sha(part)}
    if entry == "f16":
        x16 = ops.bn_apply(x, ident, relu=False, split=1, keep_fp32=False)
        y, part = ops.conv2d_fwd_f16(x16, ops.weight_pack_f16(wt), st, pad, dil, sk=sk, tile=tile)
        return {"y": _sha(y), "part": _sha(part)}
    if entry == "f16bn":
        x16 = ops.bn_apply(x, ident, relu=False, split=1, keep_fp32=False)
        ss = torch.cat([_rand(cout, seed=5) * 0.7, _rand(cout, seed=6)]).to(dev)
        res = _rand(n, ho, wo, cout, seed=7).half().to(dev)
        out = ops.conv2d_fwd_f16_bn(x16, ops.weight_pack_f16(wt), ss, res=res, relu=True, stride=st, pad=pad, dil=dil,
                                    sk=sk, tile=tile)
        return {"y": _sha(out)}
    if entry in ("x3_bnin", "f16_bnin"):
        f16 = entry == "f16_bnin"
        y_in = (_rand(n, h, w, cin, seed=8) * 3 + 1).to(dev)
        in_ss = torch.cat([_rand(cin, seed=9) * 0.7, _rand(cin, seed=10) * 2.0]).to(dev)
        wp = ops.weight_pack_f16(wt) if f16 else ops.weight_pack_x3(wt)
        y, part = ops.conv2d_fwd_bnin(y_in.half() if f16 else y_in, in_ss, wp, st, pad, dil, sk=sk, tile=tile)
        return {"y": _sha(y), "part": _sha(part)}
    dy = _rand(n, ho, wo, cout, seed=11).to(dev)
    add = _rand(n, h, w, cin, seed=12).to(dev)
    amax = ops.absmax(dy)
    dys = ops.split_pack_x3(dy, amax)
    if entry == "dgrad":
        dx = ops.conv2d_bwd_data_x3(dys, ops.weight_flip_pack_x3(wt), (n, h, w, cin), pad, dil, add=add, amax=amax,
                                    sk=sk, tile=tile)
    else:
        assert entry == "dgrad_s2" and st == 2 and dil == 1
        dx = ops.conv2d_bwd_data_x3_strided(dys, ops.weight_phase_pack_x3(wt, pad), (n, h, w, cin), (cout, k, k, cin),
                                            pad, add=add, amax=amax, sk=sk, tile=tile)
    return {"y": _sha(dx)}


def record(dev, commit):
    return {"commit": commit, "torch": torch.__version__,
            "cus": torch.cuda.get_device_properties(dev).multi_processor_count,
            "cases": {name: run_case(dev, entry, shape, tile, sk) for name, entry, shape, tile, sk, _ in CASES}}


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_device_has_the_recorded_cu_count(cuda_device, recorded):
    cus = torch.cuda.get_device_properties(cuda_device).multi_processor_count
    assert cus == recorded["cus"], ("the fixture was recorded on %d CUs and this device has %d: the plans differ, "
                                    "record the fixture again on this device" % (recorded["cus"], cus))
    assert sorted(recorded["cases"]) == sorted(c[0] for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_every_launch_has_the_recorded_bits(cuda_device, recorded, case):
    name, entry, shape, tile, sk, _ = case
    got = run_case(cuda_device, entry, shape, tile, sk)
    print(name, got)
    assert got == recorded["cases"][name], "%s: the bits differ from commit %s" % (name, recorded["commit"][:7])


def _plans(name, entry, shape, tile, sk, cus):
    """The launches [(kernel id, name, values)] the plan gives for a case (a strided dgrad: phase 0)."""
    from hkp import _lib, ops
    n, h, w, cin, cout, k, st, pad, dil = shape
    op = {"x3": _lib.HKP_KOP_FWD_X3, "w16": _lib.HKP_KOP_FWD_X3_W16, "f16": _lib.HKP_KOP_FWD_F16,
          "f16bn": _lib.HKP_KOP_FWD_F16_BN, "x3_bnin": _lib.HKP_KOP_FWD_X3, "f16_bnin": _lib.HKP_KOP_FWD_F16,
          "dgrad": _lib.HKP_KOP_DGRAD_X3, "stem_planes": _lib.HKP_KOP_STEM_X3, "stem_image": _lib.HKP_KOP_STEM_X3_IMAGE,
          "stem_u8": _lib.HKP_KOP_STEM_X3_IMAGE_U8}[entry]
    stem = entry.startswith("stem")
    d = _lib.ConvDesc(n, h, w, cin, cout, k, k, st, pad, dil, _lib.HKP_LAYOUT_NCHW if stem else _lib.HKP_LAYOUT_NHWC, tile)
    out = ops.launch_plan(d, op, sk, cus)
    if entry.endswith("_bnin"):         # the fused-input-BN entries run the halo plan on the _bnin kernels
        assert all(l["kernel"] == _lib.HKP_X3K_HALO for l in out)
        out = [dict(l, kernel=_lib.HKP_X3K_HALO_BNIN, name=l["name"].replace("_kernel<", "_bnin_kernel<")) for l in out]
    return out


def test_the_list_reaches_every_kernel_id_and_form(recorded):
    from hkp import _lib
    seen = set()
    for name, entry, shape, tile, sk, want in CASES:
        if entry == "dgrad_s2":
            continue                    # four stride-1 launches, one per phase: the plan has no descriptor for them
        plans = _plans(name, entry, shape, tile, sk, recorded["cus"])
        seen |= {l["kernel"] for l in plans}
        if want is not None and recorded["cus"] == 256:
            assert [l["name"] for l in plans] == want, name
        for key, val in FORMS.get(name, {}).items():
            if recorded["cus"] == 256:
                assert plans[0][key] == val, (name, key, plans[0][key])
    assert seen == set(range(_lib.HKP_X3K_COUNT)), "kernel ids never launched: %s" % sorted(
        set(range(_lib.HKP_X3K_COUNT)) - seen)
    large = _plans(*[c for c in CASES if c[0] == "duo_large"][0][:5], recorded["cus"])[0]
    assert large["stagger_ns"] > 0 and large["blocks"] > 2 * recorded["cus"]


if __name__ == "__main__":
    res = record(torch.device("cuda:0"), sys.argv[2])
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d cases on %d CUs" % (len(res["cases"]), res["cus"]))
