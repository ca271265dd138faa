"""The heatmap losses give the bits they gave before their kernels were folded into one
body: tests/golden/loss_bits_parent.json holds the SHA-256 of every output (loss, dheat,
plane_loss, plane_used) of tools/loss_bits.py's cases, recorded with the library of the
commit named in the file; every case is recomputed here and every hash must match.

The cross-entry tests (entry A gives the bits of entry B) cannot see a change that all entries
share; this one can.  With -ffp-contract=off and no fast-math the compiler may not reorder
the sums, so under the recorded compiler a mismatch means that the code changed an operation
order: fix the code, not the file.  Under another compiler the test fails too and says so:
regenerate the file (the tool's docstring) once the difference is understood."""
import json
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

import loss_bits  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(REPO, "tests", "golden", "loss_bits_parent.json")) as f:
        return json.load(f)


def test_the_fixture_holds_every_group(recorded):
    heads = {"topk2" if g == "topk" else g for g in loss_bits.GROUPS} | {"inputs"}
    assert {name.split()[0] for name in recorded["cases"]} == heads
    assert len(recorded["cases"]) >= 500 and len(recorded["commit"]) == 40


@pytest.mark.parametrize("group", loss_bits.GROUPS)
def test_every_output_has_the_recorded_bits(cuda_device, recorded, group):
    got = loss_bits.compute(cuda_device, group)
    head = "topk2" if group == "topk" else group
    want = {name: v for name, v in recorded["cases"].items() if name.split()[0] in (head, "inputs")}
    assert len(want) > 1 and sorted(got) == sorted(want), "the cases of %r are not those of the fixture" % group
    bad = ["%s: %s" % (name, out) for name in sorted(want) for out in sorted(want[name])
           if got[name].get(out) != want[name][out]]
    print("%s: %d cases, %d outputs differ" % (group, len(want), len(bad)))
    if not bad:
        return
    here = loss_bits.compiler_line()
    if got["inputs"] != want["inputs"]:
        why = "the seeded inputs differ (torch %s recorded): nothing can be said about the kernels" % recorded["torch"]
    elif here != recorded["compiler"]:
        why = ("the fixture records a different compiler (%r, here %r): regenerate it with tools/loss_bits.py once "
               "the difference is understood" % (recorded["compiler"], here))
    else:
        why = "the same compiler as recorded: an operation order changed; fix the code, not the fixture"
    pytest.fail("%d outputs differ from commit %s (%s); first: %s" % (len(bad), recorded["commit"][:7], why, bad[:5]))
