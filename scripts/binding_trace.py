"""The host logic of binding.Engine, recorded: what tests/test_binding_trace_cpu.py holds a rewrite of memvul_amd/binding.py to.

tests/binding_trace_kit.py has the scenarios (binding.Engine on the recorder libraries of the CPU tests: no GPU, no built library) and says what a record holds.
The file carries the commit and the sha256 of the binding.py it was recorded from; one line per scenario, so a changed call is one changed line of its diff.

  python scripts/binding_trace.py --out tests/golden/binding_trace.json     (at the commit whose behaviour is to be pinned, BEFORE binding.py is edited)

A change that means to alter what Engine calls, warns or raises records the file again; its diff then shows what moved."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import binding_trace_kit as kit  # noqa: E402
from memvul_amd import binding  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "binding_trace.json")


def dump(doc: dict, path: str):
    one = lambda v: json.dumps(v, sort_keys=True, separators=(",", ":"))  # noqa: E731
    lines = ['{"commit":%s,' % one(doc["commit"]), '"binding_sha256":%s,' % one(doc["binding_sha256"]), '"scenarios":{']
    lines += ["%s:%s%s" % (one(k), one(v), "," if i + 1 < len(doc["scenarios"]) else "") for i, (k, v) in enumerate(sorted(doc["scenarios"].items()))]
    with open(path, "w") as f:
        f.write("\n".join(lines + ["}}"]) + "\n")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--commit", help="the commit the trace belongs to (default: git rev-parse HEAD)")
    a = ap.parse_args(argv)
    commit = a.commit or subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or "unknown"
    with open(binding.__file__, "rb") as f:
        digest = hashlib.sha256(f.read()).hexdigest()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    dump({"commit": commit, "binding_sha256": digest, "scenarios": kit.run_all()}, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
