"""binding.Engine calls, warns, raises and leaves behind what it did when tests/golden/binding_trace.json was recorded (scripts/binding_trace.py): the check a
rewrite of memvul_amd/binding.py that stops at the library boundary needs.  tests/binding_trace_kit.py has the scenarios; no GPU and no built library."""
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import binding_trace as bt  # noqa: E402
import binding_trace_kit as kit  # noqa: E402

REGENERATE = "python scripts/binding_trace.py --out tests/golden/binding_trace.json   (at the commit that means to change what Engine does)"


@pytest.fixture(scope="module")
def golden():
    with open(bt.GOLDEN) as f:
        doc = json.load(f)
    assert re.fullmatch(r"[0-9a-f]{40}", doc["commit"]) and re.fullmatch(r"[0-9a-f]{64}", doc["binding_sha256"])
    return doc["scenarios"]


def test_the_scenarios_are_the_recorded_ones(golden):
    assert sorted(golden) == sorted(kit.SCENARIOS), REGENERATE


@pytest.mark.parametrize("name", list(kit.SCENARIOS))
def test_engine_does_what_was_recorded(golden, name):
    got, want = json.loads(json.dumps(kit.run(name))), golden[name]
    assert sorted(got) == sorted(want)
    for part in sorted(want):  # (part by part: the first one that differs names itself)
        assert got[part] == want[part], f"{name}: {part} differs from the record"


def test_the_record_names_every_entry_and_attributes_direct_warnings_to_the_caller(golden):
    called = {c for rec in golden.values() for c in rec["calls"]}
    assert called == kit.entries(kit.Recorder()), sorted(kit.entries(kit.Recorder()) ^ called)
    warned = [(name, w) for name, rec in golden.items() for w in rec["warnings"]]
    direct = [(name, w) for name, w in warned if w["via"] is None]
    assert len(direct) >= 20 and all(w["from_scenario_file"] for _, w in direct), [(n, w["step"]) for n, w in direct if not w["from_scenario_file"]]
    # each of the three monitors and the trip said its piece, from each of the entry points that read them directly
    for needle in ("is the most conservative form", "switched this engine to the SAFE form", "guarded form:", "exceeded the +-112 range"):
        steps = {w["step"] for _, w in direct if needle in w["text"]}
        assert {"forward", "encode", "anchor_append", "forward_by_length", "forward_by_length_end", "corpus_results"} <= steps, (needle, steps)
