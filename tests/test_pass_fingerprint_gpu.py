"""An encoder pass computes the bits it computed when tests/golden/pass_fingerprints.json was recorded (scripts/pass_fingerprint.py): the check a host-only
rewrite of engine.hip needs.  The oracle tolerances of the other GPU tests pass with a row term dropped or a GemmArgs field left over from another launch
(a few per cent of the error budget); a hash does not.  One case per handle of the script's matrix: a 2-layer model, nine batches of at most 14 rows."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

pytestmark = pytest.mark.gpu

import pass_fingerprint as pfp  # noqa: E402

REGENERATE = "python scripts/pass_fingerprint.py --out tests/golden/pass_fingerprints.json   (on an MI355X, at the commit that changed the kernels)"


@pytest.fixture(scope="module")
def golden():
    with open(pfp.GOLDEN) as f:
        doc = json.load(f)
    # the golden pins the HOST code to what these kernels were given: other kernels mean other bits for a reason this test cannot judge, and the file is recorded
    # again (its diff then shows which hashes moved) — a failure, not a skip, so that it cannot go stale unnoticed
    have = pfp.kernel_header()
    for lib in ("product", "development"):
        assert have[lib] == doc["kernel_fingerprints"][lib], \
            f"the {lib} library's kernels differ from those of commit {doc['commit']} the golden was recorded at (scripts/kernel_fingerprints.py --against " \
            f"profiles/kernel_fingerprints*.json names them): record it again with\n  {REGENERATE}"
    assert doc["kernel_classes"] == pfp.kernel_classes(), f"the kernel classes changed: {REGENERATE}"
    return doc["handles"]


@pytest.mark.parametrize("name", list(pfp.HANDLES))
def test_pass_bits_equal_the_recorded_ones(golden, name):
    assert name in golden, f"no record of handle {name}: {REGENERATE}"
    got, want = pfp.handle_record(name), golden[name]
    assert sorted(got) == sorted(want)
    diff = []
    for batch in sorted(want):
        if not isinstance(want[batch], dict):
            if got[batch] != want[batch]:
                diff.append(f"{batch}: {got[batch]} != {want[batch]}")
            continue
        assert sorted(got[batch]) == sorted(want[batch]) and all(len(got[batch][k]) == len(want[batch][k]) for k in ("taps", "launches")), batch
        diff += [f"{batch} {k}: {got[batch][k]} != {want[batch][k]}" for k in sorted(want[batch]) if k not in ("taps", "launches") and got[batch][k] != want[batch][k]]
        diff += [f"{batch} launches of class {c}: {g} != {w}" for c, g, w in zip(pfp.kernel_classes(), got[batch]["launches"], want[batch]["launches"]) if g != w]
        taps = pfp.TAPS_F32 if pfp.HANDLES[name][0] == "f32" else pfp.TAPS
        diff += [f"{batch} debug_read({buf}) after debug_encode(n_layers={n}): {g} != {w}" for (n, buf), g, w in zip(taps, got[batch]["taps"], want[batch]["taps"]) if g != w]
    assert not diff, f"{len(diff)} records of handle {name} differ from the golden (an argument of some launch changed):\n" + "\n".join(diff[:40])
