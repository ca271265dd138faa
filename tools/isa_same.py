#!/usr/bin/env python3
"""Is the device code of the working tree the same as that of a git revision?

    python tools/isa_same.py <revision>

Writes the revision's hulk-keypoints_amd/csrc/ and include/ into a temporary
directory (git archive), compiles every .hip of both trees to gfx950 assembly with
each tree's own Makefile flags plus --cuda-device-only -S, once plain (the product
library) and once with -DHKP_AB_KNOBS (the A/B library), and compares per kernel
symbol, across the whole library and not file against file:
  * the instruction text,
  * the kernel's .amdhsa_* descriptor lines,
  * its metadata entry (VGPR / AGPR / SGPR counts, LDS and scratch bytes, kernarg
    size and arguments).
Normalised out of the instruction text, and nothing else: comments, blank lines,
the debug directives (.loc, .file, .cfi_*), the numbers of local labels (.LBB<n>_,
.Lfunc_end<n>, .Ltmp<n>: they count functions and temporaries of the file), and ONE
symbol spelling, named in SPELLING below.  Fails (exit status 1) when a kernel of
the revision is missing from the working tree, a new one appears, or any compared
item differs.  A refactor that moves device code between files is accepted on this.
"""
import concurrent.futures
import glob
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("hulk-keypoints_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
JOBS = min(16, os.cpu_count() or 1)

# The one spelling difference allowed: the zero line and the NaN line of the f16x3
# convs (csrc/x3_dev.h) have internal linkage since two translation units include
# them, which mangles hkp::g_x3_zero_line as _ZN3hkpL14... instead of _ZN3hkp14...;
# the address materialisation (s_getpc + rel32 of the symbol) is otherwise the same.
SPELLING = {"_ZN3hkpL14g_x3_zero_lineE": "_ZN3hkp14g_x3_zero_lineE",
            "_ZN3hkpL13g_x3_nan_lineE": "_ZN3hkp13g_x3_nan_lineE"}

META_KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size",
             ".private_segment_fixed_size", ".kernarg_segment_size")


def makefile_flags(tree):
    """CXXFLAGS of the tree's Makefile, $(ARCH) expanded"""
    text = open(os.path.join(tree, CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    flags = re.search(r"^CXXFLAGS\s*\?=\s*(.*)$", text, re.M).group(1)
    return flags.replace("$(ARCH)", arch).split()


def compile_tree(tree, out, extra):
    """every .hip of the tree -> out/<name>.s; returns the list of (name, path)"""
    os.makedirs(out)
    flags = makefile_flags(tree) + extra + ["--cuda-device-only", "-S"]
    srcs = sorted(glob.glob(os.path.join(tree, CSRC, "*.hip")))

    def one(src):
        dst = os.path.join(out, os.path.basename(src)[:-4] + ".s")
        r = subprocess.run([HIPCC] + flags + [src, "-o", dst], capture_output=True, text=True)
        if r.returncode:
            sys.exit("compile failed: %s\n%s" % (src, r.stderr[-4000:]))
        return os.path.basename(src), dst

    with concurrent.futures.ThreadPoolExecutor(JOBS) as ex:
        return list(ex.map(one, srcs))


def normal_text(lines, spelled):
    """the instruction text of one function, normalised as the module docstring says"""
    out, tmp = [], {}
    for line in lines:
        line = line.split(";", 1)[0].strip()
        if not line or re.match(r"\.(loc|file|cfi_\w+)\b", line):
            continue
        line = re.sub(r"\.LBB\d+_", ".LBB_", line)
        line = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", line)
        line = re.sub(r"\.Ltmp\d+", lambda m: ".Ltmp%d" % tmp.setdefault(m.group(0), len(tmp)), line)
        for a, b in SPELLING.items():
            if a in line:
                line = line.replace(a, b)
                spelled[0] += 1
        out.append(line)
    return out


def entry_name(entry):
    """the kernel's own .name of a metadata entry (its arguments' names stand deeper)"""
    return next(m.group(2) for m in (re.match(r"(  - |    )\.name:\s+(\S+)", l) for l in entry) if m)


def kernels_of(path, spelled):
    """{symbol: (text, descriptor, metadata entry)} of one assembly file"""
    lines = open(path).read().split("\n")
    desc, meta, res = {}, {}, {}
    i = 0
    while i < len(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", lines[i])
        if m:
            j = i
            while ".end_amdhsa_kernel" not in lines[j]:
                j += 1
            desc[m.group(1)] = [l.split(";", 1)[0].strip() for l in lines[i:j + 1]]
            i = j
        i += 1
    # metadata: the entries of amdhsa.kernels, each from "  - " to the next
    if "amdhsa.kernels:" in lines:
        i = lines.index("amdhsa.kernels:") + 1
        entry = []
        while i < len(lines) and (lines[i].startswith("  ") or not lines[i].strip()):
            if lines[i].startswith("  - ") and entry:
                meta[entry_name(entry)] = entry
                entry = []
            entry.append(lines[i].rstrip())
            i += 1
        if entry:
            meta[entry_name(entry)] = entry
    for sym in desc:
        a = next(k for k, l in enumerate(lines) if l.startswith(sym + ":"))
        b = a
        while not re.match(r"\.Lfunc_end\d+:", lines[b]):
            b += 1
        res[sym] = (normal_text(lines[a:b + 1], spelled), desc[sym], meta[sym])
    return res


def library(files, spelled):
    """{symbol: (file, text, descriptor, metadata)} over every file of a tree"""
    lib = {}
    for name, path in files:
        for sym, rec in kernels_of(path, spelled).items():
            if sym in lib:
                sys.exit("kernel %s is defined in %s and in %s" % (sym, lib[sym][0], name))
            lib[sym] = (name,) + rec
    return lib


def counts(entry):
    got = {}
    for l in entry:
        t = l.strip().lstrip("- ").split(":")
        if t[0] in META_KEYS:
            got[t[0]] = t[1].strip()
    return " ".join("%s=%s" % (k[1:].replace("_count", "").replace("_segment", "").replace("_fixed_size", "")
                               .replace("_size", ""), got.get(k, "?")) for k in META_KEYS)


def compare(name, old, new, old_spelled, new_spelled):
    print("== %s: %d kernels in the revision, %d in the working tree" % (name, len(old), len(new)))
    print("   spelling normalised (%s): %d lines in the revision, %d in the working tree"
          % (", ".join(sorted(SPELLING)), old_spelled, new_spelled))
    bad = 0
    for sym in sorted(set(old) | set(new)):
        if sym not in new:
            print("MISSING   %s (was in %s)" % (sym, old[sym][0]))
            bad += 1
            continue
        if sym not in old:
            print("NEW       %s (in %s)" % (sym, new[sym][0]))
            bad += 1
            continue
        diff = [what for k, what in ((1, "text"), (2, "descriptor"), (3, "metadata")) if old[sym][k] != new[sym][k]]
        where = old[sym][0] if old[sym][0] == new[sym][0] else "%s -> %s" % (old[sym][0], new[sym][0])
        if diff:
            bad += 1
            print("DIFFERS   %s [%s] (%s)" % (sym, ", ".join(diff), where))
            if "text" in diff:
                a, b = old[sym][1], new[sym][1]
                k = next((k for k in range(min(len(a), len(b))) if a[k] != b[k]), min(len(a), len(b)))
                print("          %d / %d lines; first difference at line %d:\n          - %s\n          + %s"
                      % (len(a), len(b), k, a[k] if k < len(a) else "<end>", b[k] if k < len(b) else "<end>"))
        else:
            print("identical %s (%s) lines=%d %s" % (sym, where, len(new[sym][1]), counts(new[sym][3])))
    print("== %s: %s" % (name, "%d kernels, all identical" % len(new) if not bad else "%d DIFFERENCES" % bad))
    return bad


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    rev = sys.argv[1]
    sha = subprocess.run(["git", "-C", REPO, "rev-parse", rev], check=True, capture_output=True,
                         text=True).stdout.strip()
    print("revision %s (%s) against the working tree; %s" % (rev, sha, " ".join(makefile_flags(REPO))))
    bad = 0
    with tempfile.TemporaryDirectory() as td:
        old_tree = os.path.join(td, "old")
        os.makedirs(old_tree)
        ar = subprocess.run(["git", "-C", REPO, "archive", sha, CSRC, "include"], check=True, capture_output=True)
        subprocess.run(["tar", "-x", "-C", old_tree], input=ar.stdout, check=True)
        for name, extra in (("product library", []), ("A/B library (-DHKP_AB_KNOBS)", ["-DHKP_AB_KNOBS"])):
            tag = "ab" if extra else "plain"
            so, sn = [0], [0]
            old = library(compile_tree(old_tree, os.path.join(td, "s_old_" + tag), extra), so)
            new = library(compile_tree(REPO, os.path.join(td, "s_new_" + tag), extra), sn)
            bad += compare(name, old, new, so[0], sn[0])
    print("RESULT: %s" % ("identical ISA in both configurations" if not bad else "%d differences" % bad))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
