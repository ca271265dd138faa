"""Domain randomisation, host side (no GPU): the numpy restatement's Philox, the
Gaussian table, the sampler, LUT construction, the ABI structs, the argument
checks of hkp_augment_u8 (which return before any launch) and the DataLoader
worker guard."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import _augment_ref as ref
from conftest import REPO

HEADER = os.path.join(REPO, "include", "hulkkp.h")


def _hex(words):
    return " ".join("%08x" % int(w) for w in words)


def test_philox_known_answers():
    assert _hex(ref.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    ones = 0xFFFFFFFF
    assert _hex(ref.philox4x32_10((ones,) * 4, (ones, ones))) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(ref.philox4x32_10((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0))) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"
    # vectorised over counters == one at a time
    many = ref.philox4x32_10((np.arange(5, dtype=np.uint64), 0, 0, 0), (7, 9))
    for i in range(5):
        assert [int(w[i]) for w in many] == [int(w) for w in ref.philox4x32_10((i, 0, 0, 0), (7, 9))]


def test_gauss_table():
    from hkp import augment
    t = augment.gauss_table()
    assert t.dtype == np.float32 and t.shape == (4096,)
    assert np.all(np.diff(t) > 0)
    assert np.all(np.abs(t + t[::-1]) <= np.spacing(np.abs(t)))          # antisymmetric to 1 ulp
    assert abs(float(t[-1]) - 3.6683292) < 1e-6 and abs(float(t[0]) + 3.6683292) < 1e-6
    assert abs(float(np.mean(t.astype(np.float64) ** 2)) - 0.99968) < 1e-5
    assert augment.TABLE.host is t


def test_sampler_is_per_sample_and_in_range():
    from hkp import augment
    dr = augment.DomainRandomization(seed=3)
    a = dr.plan([5, 9, 2], epoch=1)
    b = dr.plan([2, 5], epoch=1)
    one = dr.plan([5], epoch=1)
    pa, pb, p1 = a.program_bytes(), b.program_bytes(), one.program_bytes()
    assert np.array_equal(pa[0], pb[1]) and np.array_equal(pa[0], p1[0]) and np.array_equal(pa[2], pb[0])
    assert np.array_equal(a.luts[0], b.luts[1]) and np.array_equal(a.luts[2], b.luts[0])
    assert dr.sample(5, 1) == augment.DomainRandomization(seed=3).sample(5, 1)
    assert dr.sample(5, 1) != dr.sample(5, 2)                              # epochs differ
    assert dr.sample(5, 1) != dr.sample(6, 1)
    assert dr.sample(5, 1) != augment.DomainRandomization(seed=4).sample(5, 1)
    assert not np.array_equal(dr.plan([5], 1).program_bytes(), dr.plan([5], 2).program_bytes())

    n = 4000
    per_channel = 0
    pos = np.zeros((8, 8), dtype=np.int64)
    for i in range(n):
        p = dr.sample(i, 0)
        assert sorted(p["order"]) == sorted(augment.OPERATORS)
        for k, name in enumerate(p["order"]):
            pos[augment.OPERATORS.index(name), k] += 1
        assert isinstance(p["hue_sat"], int) and -20 <= p["hue_sat"] <= 20
        assert all(0.85 <= x <= 1.2 for x in p["contrast"])
        if p["contrast_per_channel"]:
            per_channel += 1
            assert len(set(p["contrast"])) == 3
        else:
            assert len(set(p["contrast"])) == 1
        assert all(isinstance(x, int) and -10 <= x <= 30 for x in p["add"]) and len(p["add"]) == 3
        assert 0.85 <= p["gamma"] <= 1.2
        assert 0.0 <= p["blur"] <= 0.6
        assert 5000 <= p["temperature"] <= 35000
        assert 0.95 <= p["mul_sat"] <= 1.05
        assert 0.0 <= p["noise"] <= 0.0125 * 255
        assert all(0 <= k < 2 ** 32 for k in p["key"])
    assert 0.22 <= per_channel / n <= 0.28, per_channel / n
    assert np.all(pos > 0), pos                                            # each operator in each position
    # the integer ranges reach both ends
    hs = {dr.sample(i, 0)["hue_sat"] for i in range(n)}
    assert min(hs) == -20 and max(hs) == 20


def test_sampler_ops_argument():
    from hkp import _lib, augment
    fixed = augment.DomainRandomization(random_order=False)
    assert fixed.sample(0)["order"] == list(augment.OPERATORS)
    sub = augment.DomainRandomization(ops=["noise", "gamma"], random_order=False)
    assert sub.sample(0)["order"] == ["noise", "gamma"]
    off = augment.DomainRandomization(ops={"noise": (0, 0), "blur": (0.0, 0.0)})
    for i in range(20):
        p = off.sample(i)
        assert p["noise"] == 0.0 and p["blur"] == 0.0 and len(p["order"]) == 8
        prog = off.plan([i]).programs[0]
        kinds = [prog.stages[s].kind for s in range(prog.nstages)]
        assert prog.nstages == 6 and _lib.HKP_AUG_NOISE not in kinds and _lib.HKP_AUG_BLUR not in kinds
    assert "blur" not in augment.DomainRandomization(ops={"blur": None}).sample(0)["order"]
    with pytest.raises(ValueError):
        augment.DomainRandomization(ops=["sharpen"])
    # stage mapping of one sample
    dr = augment.DomainRandomization(seed=1, random_order=False)
    p = dr.sample(0)
    st = dr.stages(p)
    assert [s[0] for s in st] == ["hsv", "lut", "lut", "lut", "blur", "lut", "hsv", "noise"]
    assert st[0][1] == np.float32(6.0 * p["hue_sat"] / 255.0) and st[0][2] == p["hue_sat"] and st[0][3] == 1.0
    assert st[6][1:] == (0.0, 0.0, np.float32(p["mul_sat"]))
    assert st[7][2:] == p["key"]


def _rint_clamp(x):
    # float64 scalar: round half to even, clamp
    fl = math.floor(x)
    r = fl + 1 if x - fl > 0.5 else fl if x - fl < 0.5 else (fl if fl % 2 == 0 else fl + 1)
    return int(min(max(r, 0), 255))


def test_lut_construction():
    from hkp import augment
    for alpha in (0.85, 1.2):
        lut = augment.lut_contrast((alpha, 1.0, alpha))
        assert lut.shape == (3, 256) and lut.dtype == np.uint8
        for v in range(256):
            assert lut[0, v] == _rint_clamp(127.0 + alpha * (v - 127.0))
            assert lut[1, v] == v and lut[2, v] == lut[0, v]
    for a in (-10, 30):
        lut = augment.lut_add((a, 0, -a))
        for v in range(256):
            assert lut[0, v] == min(max(v + a, 0), 255) and lut[1, v] == v and lut[2, v] == min(max(v - a, 0), 255)
    for gamma in (0.85, 1.2):
        lut = augment.lut_gamma(gamma)
        for v in range(256):
            assert lut[0, v] == lut[1, v] == lut[2, v] == _rint_clamp(255.0 * (v / 255.0) ** gamma)
    for kelvin in (5000, 35000):
        m_r, m_g, m_b = augment.kelvin_multipliers(kelvin)
        lut = augment.lut_temperature(kelvin)
        for v in range(256):
            assert (lut[0, v], lut[1, v], lut[2, v]) == (_rint_clamp(v * m_b), _rint_clamp(v * m_g),
                                                          _rint_clamp(v * m_r))
    assert all(abs(m - 1.0) < 0.02 for m in augment.kelvin_multipliers(6600))
    m_r, m_g, m_b = augment.kelvin_multipliers(5000)
    assert m_r == 1.0 and m_r > m_g > m_b                                   # red-heavy
    m_r, m_g, m_b = augment.kelvin_multipliers(35000)
    assert m_b == 1.0 and m_b > m_g > m_r                                   # blue-heavy
    # the scalar formulae themselves at one point of each branch
    t = 50.0
    assert augment.kelvin_multipliers(5000) == (1.0, (99.4708025861 * math.log(t) - 161.1195681661) / 255.0,
                                                (138.5177312231 * math.log(t - 10) - 305.0447927307) / 255.0)
    t = 350.0
    assert augment.kelvin_multipliers(35000) == (329.698727446 * (t - 60) ** -0.1332047592 / 255.0,
                                                 288.1221695283 * (t - 60) ** -0.0755148492 / 255.0, 1.0)
    w0, w1, w2 = augment.blur_weights(0.6)
    assert w0.dtype == np.float32 and abs(float(w0) + 2 * float(w1) + 2 * float(w2) - 1.0) < 1e-7
    e = [math.exp(-k * k / (2 * 0.36)) for k in range(3)]
    assert w1 == np.float32(e[1] / (e[0] + 2 * e[1] + 2 * e[2]))
    assert augment.blur_weights(0.001) == (1.0, 0.0, 0.0)


def _header_struct(name):
    """[(field, ctype, count)] of `typedef struct <name> { ... }` in the header."""
    text = open(HEADER).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    macros = {m: int(v) for m, v in re.findall(r"#define (HKP_AUG_[A-Z_]+) (\d+)", text)}
    out = []
    for typ, field, cnt in re.findall(r"(\w+)\s+(\w+)(?:\[(\w+)\])?;", body):
        out.append((field, typ, 1 if not cnt else int(macros.get(cnt, cnt))))
    return out, macros


def test_struct_layout_matches_header():
    from hkp import _lib, augment
    size = {"int32_t": 4, "uint32_t": 4, "float": 4, "hkp_aug_stage": 32}
    for cname, mirror in (("hkp_aug_stage", _lib.AugStage), ("hkp_aug_program", _lib.AugProgram)):
        fields, macros = _header_struct(cname)
        assert [f for f, _, _ in fields] == [f for f, _ in mirror._fields_]
        off = 0
        for field, typ, cnt in fields:                  # every member is 4-byte aligned: no padding
            assert getattr(mirror, field).offset == off, (cname, field)
            assert getattr(mirror, field).size == size[typ] * cnt, (cname, field)
            off += size[typ] * cnt
        assert ctypes.sizeof(mirror) == off
    assert ctypes.sizeof(_lib.AugStage) == 32 and ctypes.sizeof(_lib.AugProgram) == 288
    for k in ("LUT", "HSV", "BLUR", "NOISE", "MAX_STAGES", "GAUSS_TABLE", "TILE_H", "TILE_W"):
        assert macros["HKP_AUG_" + k] == getattr(_lib, "HKP_AUG_" + k)
    assert (augment.TILE_H, augment.TILE_W) == (macros["HKP_AUG_TILE_H"], macros["HKP_AUG_TILE_W"])


def test_bad_arguments_raise_without_launch():
    """Null pointers stand in for the device buffers elsewhere: every call here has to
    return from the argument checks (it would fault, or need a GPU, otherwise)."""
    from hkp import _lib, augment
    P = ctypes.c_void_p
    plan = augment.Plan.from_stages([[("hsv", 0.1, 2.0, 1.0)], []])
    good = dict(n=2, h=8, w=8, img_in=P(4096), img_out=P(8192), host=plan.programs, dev=P(256), luts=P(512),
                table=P(1024))

    def call(**kw):
        a = dict(good, **kw)
        return _lib.call("hkp_augment_u8", a["n"], a["h"], a["w"], a["img_in"], a["img_out"], a["host"], a["dev"],
                         a["luts"], a["table"], None)

    for kw in (dict(h=2), dict(w=2), dict(h=0), dict(w=-1)):
        with pytest.raises(_lib.HkpError, match="at least 3"):
            call(**kw)
    with pytest.raises(_lib.HkpError, match="batch size"):
        call(n=0)
    for name in ("img_in", "img_out", "dev", "luts", "table"):
        with pytest.raises(_lib.HkpError, match="null pointer"):
            call(**{name: None})
    with pytest.raises(_lib.HkpError, match="null pointer"):
        call(host=None)
    with pytest.raises(_lib.HkpError, match="overlap"):
        call(img_out=P(4096))                                   # in place
    with pytest.raises(_lib.HkpError, match="overlap"):
        call(img_out=P(4096 + 100))                             # partly overlapping (2*8*8*3 = 384 bytes)
    with pytest.raises(_lib.HkpError, match="aligned"):
        call(luts=P(513))

    def programs(edit):
        p = augment.Plan.from_stages([[("hsv", 0.1, 2.0, 1.0)], [("blur", 0.5, 0.25, 0.0), ("noise", 1.0, 1, 2)]])
        edit(p.programs)
        return p.programs

    def count_hi(p):
        p[1].nstages = _lib.HKP_AUG_MAX_STAGES + 1

    def count_lo(p):
        p[0].nstages = -1

    def kind_bad(p):
        p[1].stages[1].kind = 5

    def kind_zero(p):
        p[0].stages[0].kind = 0

    def two_blurs(p):
        p[1].stages[1].kind = _lib.HKP_AUG_BLUR

    for edit, msg in ((count_hi, "stage count"), (count_lo, "stage count"), (kind_bad, "unknown stage kind"),
                      (kind_zero, "unknown stage kind"), (two_blurs, "more than one BLUR")):
        with pytest.raises(_lib.HkpError, match=msg):
            call(host=programs(edit))
    # the packer refuses the same programs earlier
    with pytest.raises(_lib.HkpError, match="one BLUR"):
        augment.Plan.from_stages([[("blur", 1.0, 0.0, 0.0), ("blur", 1.0, 0.0, 0.0)]])
    with pytest.raises(_lib.HkpError, match="at most"):
        augment.Plan.from_stages([[("hsv", 0.0, 0.0, 1.0)] * 9])


def test_ops_wrapper_checks_on_host():
    import torch
    from hkp import _lib, augment, ops
    plan = augment.Plan.from_stages([[]])
    with pytest.raises(_lib.HkpError, match="GPU"):            # no CPU path
        ops.augment_u8(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), plan)


def test_call_in_loader_worker_raises(monkeypatch):
    import torch
    from hkp import _lib, augment
    monkeypatch.setattr(torch.utils.data, "get_worker_info", lambda: object())
    dr = augment.DomainRandomization()
    with pytest.raises(_lib.HkpError, match=r"DeviceBatches\(augment="):
        dr(np.zeros((8, 8, 3), dtype=np.uint8))


def test_restatement_identities():
    """Properties of the numpy restatement itself (what the GPU tests compare against)."""
    from hkp import augment
    from oracle import recipe
    img = recipe.seeded_images_u8(1, 9, 11, 3)[0]
    ident = np.tile(np.arange(256, dtype=np.uint8), (3, 1))
    assert np.array_equal(ref.stage_lut(img, ident), img)
    assert np.array_equal(ref.stage_blur(img, 1.0, 0.0, 0.0), img)
    assert np.array_equal(ref.stage_noise(img, 0.0, (1, 2), augment.gauss_table()), img)
    # a flat image stays flat under the blur, whatever the weights' rounding
    flat = np.full((5, 7, 3), 200, dtype=np.uint8)
    assert np.array_equal(ref.stage_blur(flat, *augment.blur_weights(0.6)), flat)
    # greys pass a hue shift and a saturation scale unchanged (an added saturation tints
    # them, as S' = S + a says); a saturation of zero turns a colour grey
    grey = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2)
    assert np.array_equal(ref.stage_hsv(grey, 0.47, 0.0, 1.05), grey)
    assert not np.array_equal(ref.stage_hsv(grey, 0.0, 20.0, 1.0), grey)
    red = np.array([[[0, 0, 255]]], dtype=np.uint8)
    assert ref.stage_hsv(red, 0.0, -255.0, 1.0).tolist() == [[[255, 255, 255]]]
    assert ref.stage_hsv(red, 2.0, 0.0, 1.0).tolist() == [[[0, 255, 0]]]            # +2 sectors: green
    assert ref.stage_hsv(red, -2.0, 0.0, 1.0).tolist() == [[[255, 0, 0]]]           # wraps: blue
