"""Per-kernel fingerprints of the library's device code (memvul_amd/build.py kernel_fingerprints): print them, write them, or compare them with a
recorded map.

  python scripts/kernel_fingerprints.py [--dev | --tok | --pp | --retrieve | --claims | --bank | --rank] [--lib FILE.so] [--out FILE.json] [--against FILE.json]

--against lists the symbols that were added, removed or changed and exits 1 if there are any: a host-only edit of engine.hip or of its parts must report none, for the
product and for the development build (profiles/kernel_fingerprints*.json hold the maps of the tree as committed; --tok: libmemvul_tok_u8.so, the UTF-8 tokenise
kernel's own library, profiles/kernel_fingerprints_tok.json; --retrieve: libmemvul_retrieve.so, per-anchor retrieval; --claims: libmemvul_claims.so, per-anchor claims;
--bank: libmemvul_bank.so, the anchor-bank audit; --rank: libmemvul_rank.so, per-anchor ranking quality, profiles/kernel_fingerprints_rank.json)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from memvul_amd import build  # noqa: E402


def diff(old: dict, new: dict) -> list:
    lines = ["added   " + k for k in sorted(set(new) - set(old))]
    lines += ["removed " + k for k in sorted(set(old) - set(new))]
    lines += ["changed " + k for k in sorted(set(old) & set(new)) if old[k] != new[k]]
    return lines


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--dev", action="store_true", help="the development build (libmemvul_hip_dev.so)")
    ap.add_argument("--tok", action="store_true", help="the UTF-8 tokenise kernel's library (libmemvul_tok_u8.so)")
    ap.add_argument("--pp", action="store_true", help="the fixed-form persistent GEMMs' library (libmemvul_pp_fixed.so; profiles/kernel_fingerprints_pp.json)")
    ap.add_argument("--retrieve", action="store_true", help="the per-anchor retrieval library (libmemvul_retrieve.so)")
    ap.add_argument("--claims", action="store_true", help="the per-anchor claims library (libmemvul_claims.so)")
    ap.add_argument("--bank", action="store_true", help="the anchor-bank audit library (libmemvul_bank.so)")
    ap.add_argument("--rank", action="store_true", help="the per-anchor ranking library (libmemvul_rank.so)")
    ap.add_argument("--lib", help="another library file")
    ap.add_argument("--against", help="a map written by --out: compare, exit 1 on any difference")
    ap.add_argument("--out", help="write the map here instead of printing it")
    a = ap.parse_args(argv)
    side = [key for key in reversed(list(build.SIDE_LIBS)) if getattr(a, key)]  # (several flags: the last of the table wins, as before)
    fp = build.kernel_fingerprints(a.lib or (build.side_lib_path(side[0]) if side else build.LIB_PATH_DEV if a.dev else build.LIB_PATH))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(fp, f, indent=0, sort_keys=True)
            f.write("\n")
    elif not a.against:
        json.dump(fp, sys.stdout, indent=0, sort_keys=True)
        print()
    if a.against:
        with open(a.against) as f:
            lines = diff(json.load(f), fp)
        print("\n".join(lines) if lines else f"{len(fp)} symbols, no difference")
        return 1 if lines else 0
    return 0


if __name__ == "__main__":
    sys.exit(main())
