"""The launch plan of the f16x3 / plain-fp16 convs (csrc/x3_plan.h, hkp_conv_x3_launch_plan),
checked without a GPU:

  * the kernel names and the BN-partial layouts it gives are those of the library before the
    plan existed, over every case of cases(): tests/golden/x3_plan_parent.json was recorded
    with that commit's library (`python tests/test_x3_plan_cpu.py` writes it; no device, so
    the planner saw 256 CUs), and hkp_conv_kernel_name / hkp_conv_x3_stat_layout are the
    plan's first launch / its segments;
  * the plan's geometry: the launches cover every tile once, tails, stream-K grids, mix
    regions, workspace use, at 64, 256 and 304 CUs;
  * x3_plan.h alone, with the host compiler and the address / undefined-behaviour
    sanitizers, swept out to M = 2^31 - 1."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "hulk-keypoints_amd"), os.path.join(REPO, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from hkp import _lib  # noqa: E402

FIXTURE = os.path.join(REPO, "tests", "golden", "x3_plan_parent.json")
POLICIES = tuple(range(18)) + (99,)
# hkp_conv_kernel_name's ops before HKP_KOP_FWD_F16_BN: forwards, dgrad, wgrad, the stem's three
OPS = (_lib.HKP_KOP_FWD_X3, _lib.HKP_KOP_FWD_X3_W16, _lib.HKP_KOP_FWD_X3_X16, _lib.HKP_KOP_FWD_F16,
       _lib.HKP_KOP_DGRAD_X3, _lib.HKP_KOP_WGRAD_X3, _lib.HKP_KOP_STEM_X3, 7, 8)
GEMM_OPS = OPS[:5]
EDGE_M = {1: (1, 1), 255: (15, 17), 256: (16, 16), 257: (1, 257), 65536: (256, 256), 65537: (1, 65537),
          76800: (240, 320), 153600: (480, 320)}
STEMS = [(32, 480, 640, 3, 64, 7, 2, 3, 1), (2, 120, 160, 3, 64, 7, 2, 3, 1), (1, 16, 64, 3, 64, 7, 2, 3, 1)]


def shapes():
    """(n, h, w, cin, cout, k, stride, pad, dil) of every case, in a fixed order, no repeats."""
    import test_gpu_mix_tiles as mix
    import test_gpu_precision as prec
    out = []
    with open(os.path.join(REPO, "hulk-keypoints_amd", "hkp", "tile_plan.json")) as f:
        for key in json.load(f)["shapes"]:
            out.append(tuple(int(v) for v in key.split("|")[1:]))
    out += [c[1:] for c in prec.TAIL_CASES] + prec.A3_192_CASES + prec.BODY_CASES + prec.SK_CASES
    out += [(n, h, w, ci, co, 3, 1, 1, 1) for n, h, w, ci, co in prec.HALO_CASES + prec.BNIN_CASES]
    out += [c for c, _ in mix.MIX_CASES]
    for m, (h, w) in EDGE_M.items():
        for cin in (32, 64, 256):
            for cout in (64, 128, 256, 512):
                out += [(1, h, w, cin, cout, 1, 1, 0, 1), (1, h, w, cin, cout, 3, 1, 1, 1)]
    out += STEMS
    seen, uniq = set(), []
    for s in out:
        if tuple(s) not in seen:
            seen.add(tuple(s))
            uniq.append(tuple(s))
    return uniq


def desc(shape, tile):
    n, h, w, cin, cout, k, st, pad, dil = shape
    return _lib.ConvDesc(n, h, w, cin, cout, k, k, st, pad, dil,
                         _lib.HKP_LAYOUT_NCHW if shape in STEMS else _lib.HKP_LAYOUT_NHWC, tile)


def cases():
    """(shape, policy, op) of every case; each is asked with and without a stream-K workspace."""
    return [(s, t, op) for s in shapes() for t in POLICIES for op in OPS]


_buf = ctypes.create_string_buffer(128)
_seg = (ctypes.c_int32 * 6)()


def _name(d, op, sk):
    n = _lib.lib().hkp_conv_kernel_name(ctypes.byref(d), op, sk, _buf, 128)
    return _buf.value.decode() if n >= 0 else n


def answers(shape, tile, op):
    """What the name and layout queries say: (name or error without a workspace, with one,
    [segment count or error, segments...], rows per statistic tile)."""
    d = desc(shape, tile)
    n = _lib.lib().hkp_conv_x3_stat_layout(ctypes.byref(d), op, _seg)
    lay = [n] + (list(_seg[:2 * n]) if n > 0 else [])
    return (_name(d, op, 0), _name(d, op, 1), lay, _lib.lib().hkp_conv_x3_stat_tile_rows(ctypes.byref(d), op))


def _plan(d, op, sk, cus, i=0):
    """(launch count or error, name, out[]) of launch i."""
    out = (ctypes.c_int64 * _lib.HKP_X3_LAUNCH_PLAN_LEN)()
    n = _lib.lib().hkp_conv_x3_launch_plan(ctypes.byref(d), op, sk, cus, i, _buf, 128, out)
    return n, (_buf.value.decode() if n >= 0 else None), out


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        doc = json.load(f)
    doc["table"] = [(a, b, lay, rows) for a, b, lay, rows in doc["table"]]
    return doc


def test_names_and_layouts_are_the_parents(recorded):
    """4a: every case answers as the parent commit's library did, and the name and layout
    queries are readings of the plan."""
    assert [list(s) for s in shapes()] == recorded["shapes"], \
        "the case list changed (tile_plan.json or a GPU test's shape list): record the fixture again"
    cs = cases()
    assert len(cs) == len(recorded["cases"])
    names = recorded["names"]
    bad = []
    for (shape, tile, op), idx in zip(cs, recorded["cases"]):
        a, b, lay, rows = recorded["table"][idx]
        want = (a if a < 0 else names[a], b if b < 0 else names[b], lay, rows)
        got = answers(shape, tile, op)
        if (got[0], got[1], got[2], got[3]) != want:
            bad.append((shape, tile, op, got, want))
            continue
        d = desc(shape, tile)
        for sk in (0, 1):
            for cus in (256, 0):           # 256 explicitly, and the library's own count (256 without a device)
                n, name, out = _plan(d, op, sk, cus)
                if (name if n >= 0 else n) != got[sk]:
                    bad.append((shape, tile, op, sk, cus, "plan launch 0", name, n, got[sk]))
            if sk == 1 and lay[0] > 0 and n >= 0:
                segs = [out[28]] + list(out[22:22 + 2 * out[28]])
                if segs != lay:
                    bad.append((shape, tile, op, "segments", segs, lay))
    assert not bad, "%d of %d cases differ; first: %s" % (len(bad), len(cs), bad[:3])


# (getattr: the recorder below also runs on the library from before the plan existed)
F = {name: i for i, name in enumerate(getattr(_lib, "X3_LAUNCH_FIELDS", ()))}
SEG, NSEG, CUS, M_, MT, BN, BM = 22, 28, 29, 30, 31, 32, 33


def _ws_cap(cus):
    return (64 << 10) + 2 * cus * 256 * 1024        # hkp_conv_x3_sk_workspace_bytes() on cus CUs


def _check_geometry(shape, tile, op, sk, cus):
    """4b for one plan; returns the kernel ids it launches."""
    d = desc(shape, tile)
    n, _, o = _plan(d, op, sk, cus)
    if n <= 0:
        return ()
    ls = [o] + [_plan(d, op, sk, cus, i)[2] for i in range(1, n)]
    what = (shape, tile, op, sk, cus)
    m, mt, bn, bm, nt, nks = o[M_], o[MT], o[BN], o[BM], o[F["n_tiles"]], o[F["nks"]]
    kout = shape[3] if op == _lib.HKP_KOP_DGRAD_X3 else shape[4]
    assert o[CUS] == cus and mt == (m + 255) // 256 and nt * bn == kout and nt >= 1 and nks >= 1, what
    kern = [l[F["kernel"]] for l in ls]
    for l in ls:
        assert l[F["threads"]] == (256 if l[F["kernel"]] == _lib.HKP_X3K_DUO else 512), what
        assert l[F["blocks"]] < 2 ** 31, what
        if not sk:
            assert not l[F["uses_ws"]] and l[F["ws_bytes"]] == 0, what
        if l[F["uses_ws"]]:
            assert 0 < l[F["ws_bytes"]] <= _ws_cap(cus), what
    rm = mt * nt // cus * cus // nt                 # m-tiles of the full rounds
    tm = mt - rm

    def tail(groups, first, units, blocks):         # a tail of `groups` groups from m-tile `first`
        assert first == rm and tm > 0 and units == tm * nks and blocks == groups * nt, what
        assert groups % tm == 0 and groups * nt <= cus and groups <= units, what
        s = groups // tm
        for g in (0, 1, s - 1, s, groups - 1):      # every group's units [g U / NG, (g + 1) U / NG) inside one m-tile
            if 0 <= g < groups:
                u0, u1 = g * units // groups, (g + 1) * units // groups
                assert u0 < u1 and u0 // nks == (u1 - 1) // nks == g // s, (what, g)

    if kern[0] == _lib.HKP_X3K_A3_MIX:
        mp = (ctypes.c_int32 * _lib.HKP_MIX_PLAN_LEN)()
        assert _lib.lib().hkp_conv_x3_mix_plan(m, nt, cus, mp) >= 1 and n == 1, what
        mts, base, part = mp[4:7], mp[7:10], mp[10:13]
        assert (o[F["mix_b1"]], o[F["mix_b2"]]) == (mts[0] * nt, (mts[0] + mts[1]) * nt), what
        assert (o[F["mix_m1"]], o[F["mix_m2"]], o[F["mix_p1"]], o[F["mix_p2"]]) == (base[1], base[2], part[1], part[2]), what
        assert o[F["blocks"]] == sum(mts) * nt and not o[F["uses_ws"]], what
        assert sum(o[SEG + 2 * i + 1] for i in range(o[NSEG])) == mp[13], what
    elif bm != 256:
        assert n == 1 and o[F["blocks"]] == (m + bm - 1) // bm * nt and not o[F["uses_ws"]], what
        assert kern[0] in (_lib.HKP_X3K_A3_192, _lib.HKP_X3K_A3_160, _lib.HKP_X3K_A3_160X128), what
        assert list(o[SEG:SEG + 2]) == [bm // 2, (m + bm // 2 - 1) // (bm // 2)], what
    elif kern[0] in (_lib.HKP_X3K_SK_128, _lib.HKP_X3K_SK_64):
        units = o[F["sk_units"]]
        assert n == 1 and units == mt * nks and o[F["uses_ws"]] and not o[F["sk_one"]], what
        assert o[F["blocks"]] == min(cus // nt, units) * nt and 0 < o[F["blocks"]] // nt <= units, what
    elif n == 2:
        main, t = ls
        assert kern[1] == _lib.HKP_X3K_TAIL and kern[0] in (_lib.HKP_X3K_TILE_256, _lib.HKP_X3K_A3), what
        assert main[F["blocks"]] == rm * nt and not main[F["uses_ws"]] and main[F["mt0"]] == 0, what
        assert t[F["sk_one"]] == 1 and t[F["uses_ws"]], what
        tail(t[F["blocks"]] // nt, t[F["mt0"]], t[F["sk_units"]], t[F["blocks"]])
    elif o[F["tail_groups"]]:
        assert kern[0] == _lib.HKP_X3K_A3 and o[F["sk_one"]] == 1 and o[F["uses_ws"]], what
        assert o[F["main_blocks"]] == rm * nt, what
        tail(o[F["tail_groups"]], o[F["tail_mt0"]], o[F["tail_units"]], o[F["blocks"]] - o[F["main_blocks"]])
    else:                                           # one 256-row tile per block
        assert n == 1 and o[F["blocks"]] == mt * nt and not o[F["uses_ws"]] and o[F["main_blocks"]] == 0, what
        assert o[F["sk_units"]] == 0 and o[F["mt0"]] == 0, what
    if kern[0] == _lib.HKP_X3K_DUO:
        assert o[F["stagger_blocks"]] == 2 * cus and (o[F["stagger_ns"]] > 0) == (o[F["blocks"]] > 2 * cus), what
    else:
        assert o[F["stagger_blocks"]] == cus and o[F["stagger_ns"]] == -1, what
    return tuple(kern)


@pytest.mark.parametrize("cus", [64, 256, 304])
def test_plan_geometry(cus):
    """4b: every forward and dgrad plan covers its tiles once, with sound tails, stream-K grids,
    mix regions and workspace use."""
    assert _lib.lib().hkp_conv_x3_sk_workspace_bytes() == _ws_cap(256)      # no device here: 256 CUs
    seen = set()
    for shape, tile, op in cases():
        if op in GEMM_OPS:
            for sk in (0, 1):
                seen |= set(_check_geometry(shape, tile, op, sk, cus))
    # every kernel of the launcher but the fused-input-BN twin of the halo body (no op names it) and the stem's
    assert seen == set(range(_lib.HKP_X3K_HALO_BNIN)) | {_lib.HKP_X3K_DUO}, sorted(seen)


def _first(shape, op=_lib.HKP_KOP_FWD_X3, tile=0, sk=1, cus=256):
    from hkp import ops
    n, h, w, cin, cout, k, st, pad, dil = shape
    return ops.launch_plan(_lib.ConvDesc(n, h, w, cin, cout, k, k, st, pad, dil, 0, tile), op, sk, cus)


def test_pinned_plans():
    """Plans worked out by hand from the code before the plan existed (256 CUs, AUTO, stream-K on)."""
    (a,) = _first((32, 60, 80, 256, 256, 3, 1, 2, 2))
    assert (a["m_tiles"], a["name"], a["main_blocks"], a["tail_groups"], a["tail_mt0"], a["tail_units"], a["blocks"]) == \
        (600, "conv_x3_a3_kernel<3>", 512, 176, 512, 88 * 72, 688)
    (b,) = _first((32, 60, 80, 512, 512, 3, 1, 4, 4))
    assert (b["blocks"], b["tail_groups"], b["main_blocks"], b["uses_ws"]) == (1200, 0, 0, 0)
    (c,) = _first((4, 60, 80, 256, 256, 3, 1, 2, 2))
    assert (c["m_tiles"], c["main_blocks"], c["tail_groups"], c["blocks"]) == (75, 0, 225, 225)
    two = _first((32, 60, 80, 256, 256, 3, 1, 2, 2), tile=_lib.HKP_TILE_256_TAIL)
    assert len(two) == 2 and two[1]["name"] == "conv_x3_tail_kernel<256, 3>"
    assert two[0]["name"] == "conv_x3_kernel<256, false, false, 16, false, 3>" and two[0]["blocks"] == 512
    layer1 = (128, 120, 160, 64, 64, 3, 1, 1, 1)
    assert _first(layer1, _lib.HKP_KOP_FWD_F16)[0]["name"] == "conv_x3_halo_kernel<1>"
    fused = _first(layer1, _lib.HKP_KOP_FWD_F16_BN)[0]["name"]      # its fused output BN rules the halo body out
    assert "halo" not in fused and fused.startswith("conv_x3_"), fused
    d = _lib.ConvDesc(*layer1[:5], 3, 3, 1, 1, 1, 0, 0)
    assert _lib.lib().hkp_conv_x3_stat_layout(ctypes.byref(d), _lib.HKP_KOP_FWD_F16_BN, _seg) < 0
    assert _lib.lib().hkp_conv_x3_stat_tile_rows(ctypes.byref(d), _lib.HKP_KOP_FWD_F16_BN) == 128


SWEEP = r"""
#include "x3_plan.h"
using namespace hkp;
int main() {
    const long Ms[] = {1, 255, 256, 257, 65536, 65537, 76800, 153600, (1L << 31) - 1};
    const int cins[] = {32, 64, 256}, couts[] = {64, 128, 256, 512}, cuss[] = {1, 8, 256, 304};
    const int policies[] = {0, 1, 2, 3, 4, 5, 6, 9, 10, 11, 12, 13, 15, 16, 17};
    long plans = 0, blocks = 0;
    for (long M : Ms) for (int cin : cins) for (int cout : couts) for (int k = 1; k <= 3; k += 2)
    for (int cus : cuss) for (int policy : policies) for (int P = 1; P <= 4; ++P) for (int sk = 0; sk < 2; ++sk)
    for (int dgrad = 0; dgrad < 2; ++dgrad) {
        if (cin % (x3_packed(P) ? 32 : 64) || (dgrad && (P != 3 || cin % 64))) continue;
        hkp_conv_desc d = {1, 1, (int32_t)M, cin, cout, k, k, 1, k / 2, 1, HKP_LAYOUT_NHWC, policy};
        if (M == 76800) { d.h = 240; d.w = 320; }
        const X3Problem p = dgrad ? x3_problem_dgrad(&d, d.h, d.w) : x3_problem_fwd(&d, d.h, d.w, P);
        const X3LaunchPlan pl = x3_launch_plan(p, policy, sk ? x3_sk_ws_bytes(256, cus) : 0, cus);
        if (pl.n_launches < 1 || pl.n_launches > 2 || pl.n_seg < 1 || pl.n_seg > 3) return 1;
        char name[128];
        for (int i = 0; i < pl.n_launches; ++i) {
            if (x3_kernel_name(pl.launch[i].kernel, P, name, sizeof name) <= 0 || pl.launch[i].blocks < 0) return 2;
            blocks += pl.launch[i].blocks;
        }
        ++plans;
    }
    X3Problem ph;
    int col_pad = 0;
    hkp_conv_desc s2 = {2, 31, 33, 64, 128, 3, 3, 2, 1, 1, HKP_LAYOUT_NHWC, 0};
    for (int py = 0; py < 2; ++py) for (int px = 0; px < 2; ++px)
        if (x3_problem_dgrad_phase(&s2, 16, 17, py, px, &ph, &col_pad)) plans += x3_launch_plan(ph, 0, 0, 256).n_launches;
    printf("%ld plans, %ld blocks\n", plans, blocks);
    return plans > 0 ? 0 : 3;
}
"""


def test_header_stands_alone_under_sanitizers(tmp_path):
    """4c: x3_plan.h needs no GPU runtime — a host-only program that includes nothing else
    sweeps x3_launch_plan under ASan + UBSan and exits 0."""
    cxx = next((c for c in ("g++", "clang++", "/opt/rocm/llvm/bin/clang++") if subprocess.run(
        ["sh", "-c", "command -v %s" % c], capture_output=True).returncode == 0), None)
    assert cxx, "no host C++ compiler"
    src = tmp_path / "sweep.cc"
    src.write_text(SWEEP)
    exe = str(tmp_path / "sweep")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "hulk-keypoints_amd", "csrc"), str(src), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    print(run.stdout.strip())


if __name__ == "__main__":                          # record the fixture (with the parent commit's library)
    table, index, names, nidx, flat = [], {}, [], {}, []

    def nid(v):
        if not isinstance(v, str):
            return v
        if v not in nidx:
            nidx[v] = len(names)
            names.append(v)
        return nidx[v]

    for shape, tile, op in cases():
        a, b, lay, rows = answers(shape, tile, op)
        key = (nid(a), nid(b), tuple(lay), rows)
        if key not in index:
            index[key] = len(table)
            table.append([key[0], key[1], lay, rows])
        flat.append(index[key])
    commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=REPO, capture_output=True, text=True).stdout.strip()
    with open(sys.argv[1] if len(sys.argv) > 1 else FIXTURE, "w") as f:
        json.dump({"commit": commit, "shapes": [list(s) for s in shapes()], "names": names, "table": table,
                   "cases": flat}, f, separators=(",", ":"))
        f.write("\n")
    print("%d cases, %d distinct answers, %d names" % (len(flat), len(table), len(names)))
