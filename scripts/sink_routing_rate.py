"""Rate of the guarded form with and without a sink-token list, and of the safe form, against the share of sequences that carry the listed token (GPU;
DESIGN.md section 2, "The sink-token list").

The workload of scripts/guarded_form_rates.py: a resident corpus of 256-token issue reports on the sink model mid_all_80_3001 (gains from
tests/golden/r06_sink_refs.npz), swept in batches of 256, the share f = 0, 1/16, 1/4, 1 of the rows marked with the sink token (synth.MID_ID at len // 2, the
same share in every batch) and every other occurrence of that token replaced; the bank is the case's six marked anchors.  Per round and share, alternating on
one GPU: the guarded form without a list, the guarded form with the list [MID_ID], the safe form — issue reports/s of the best of two timed sweeps
(corpus_run + corpus_results: the rescoring is inside) after one that warms up.  With --parent-tree DIR (a checkout of the parent commit with its library
built) every round also times that tree's guarded form at f = 0, in a child process.

Printed: every figure, per (share, configuration) the mean over the rounds and the spread (max - min) between them, the model 1 + 0.34 f_r + 1.34 f_s next to
what was measured, and the two statements the change is held to:
  A. at f = 0 the list-carrying engine is within the repeat-to-repeat spread of the parent's guarded form;
  B. with the list the guarded form is never slower than without it at the same f, beyond that spread.
Usage: python scripts/sink_routing_rate.py [--rows 4096] [--rounds 3] [--parent-tree DIR]"""
import argparse
import json
import os
import subprocess
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARES = (0.0, 1 / 16, 1 / 4, 1.0)
CONFIGS = ("guarded", "routed", "safe")  # routed = guarded + the list


def _tree(argv):
    return argv[argv.index("--tree") + 1] if "--tree" in argv else ROOT


sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, _tree(sys.argv))  # (a worker of --parent-tree imports THAT tree's memvul_amd; the model and the ids are the same arrays either way)


def workload(rows, S=256):
    from memvul_amd import synth
    import r06_make_sink_refs as mk6

    refs = np.load(os.path.join(ROOT, "tests", "golden", "r06_sink_refs.npz"))
    dims, w, _, _, aids, alens = mk6.case("mid", "all", 0.8, 3001, gains=refs["mid_all_80_3001_gains"])[:6]
    base, lens = synth.make_ids(rows, S, dims.vocab_size, seed=synth.SEED + 31, ragged=False)
    base[base == synth.MID_ID] = synth.MID_ID + 1
    corpora = {}
    for f in SHARES:
        ids = base.copy()
        marked = np.arange(rows)[np.arange(rows) % 16 < round(16 * f)]  # the same share in every batch
        if len(marked):
            ids[marked] = synth.mark_mid_token(ids[marked], lens[marked])
        corpora[f] = ids
    return dims, w, aids, alens, corpora, lens


def engine(dims, w, form, batch, aids, alens, tokens=None, S=256):
    from memvul_amd.binding import Engine

    eng = Engine(0, vocab_size=dims.vocab_size, layers=12, max_tokens=batch * S, max_batch=batch, max_anchors=16)
    eng.load_state_dict(w, "precise")
    eng.set_form(form)
    if tokens:
        eng.set_sink_tokens(tokens)
    for g in range(len(alens)):
        eng.anchor_append(aids[g:g + 1, :int(alens[g])], alens[g:g + 1])
    return eng


def sweep_rate(eng, ids, lens, batch, timed=2):
    n = len(lens)
    eng.corpus_upload(ids, lens)
    best = None
    for it in range(timed + 1):  # (the first sweep warms up — and computes the corpus' route flags, once per upload)
        eng.form_stats(reset=True)
        if hasattr(eng, "route_stats"):
            eng.route_stats(reset=True)
        eng.sync()
        t0 = time.perf_counter()
        eng.corpus_run(0, n, batch)
        eng.corpus_results(0, n)
        t = time.perf_counter() - t0
        if it:
            best = t if best is None else min(best, t)
    seqs, resc = eng.form_stats()
    return n / best, resc, (eng.route_stats() if hasattr(eng, "route_stats") else 0)


def worker(args):
    """The guarded form of the tree given with --tree at f = 0: one JSON line."""
    warnings.simplefilter("ignore")
    dims, w, aids, alens, corpora, lens = workload(args.rows)
    eng = engine(dims, w, "guarded", args.batch, aids, alens)
    rate, resc, _ = sweep_rate(eng, corpora[0.0], lens, args.batch)
    eng.close()
    print(json.dumps({"rate": rate, "rescored": resc}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--tree", default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    from memvul_amd import synth

    warnings.simplefilter("ignore")  # (the guarded form warns about the rescored share: that is what is measured here)
    dims, w, aids, alens, corpora, lens = workload(args.rows)
    engs = {"guarded": engine(dims, w, "guarded", args.batch, aids, alens), "routed": engine(dims, w, "guarded", args.batch, aids, alens, [synth.MID_ID]),
            "safe": engine(dims, w, "safe", args.batch, aids, alens)}
    rates = {}
    for rnd in range(args.rounds):
        print("== round %d" % (rnd + 1), flush=True)
        if args.parent_tree:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--tree", args.parent_tree, "--rows", str(args.rows), "--batch", str(args.batch)],
                               capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                print(r.stdout, r.stderr)
                raise SystemExit("the parent tree's worker failed")
            got = json.loads(r.stdout.strip().splitlines()[-1])
            rates.setdefault((0.0, "parent guarded"), []).append(got["rate"])
            print("f = %-6.4g %-14s %8.0f issue reports/s   rescored %d" % (0.0, "parent guarded", got["rate"], got["rescored"]), flush=True)
        for f in SHARES:
            for c in CONFIGS:
                rate, resc, routed = sweep_rate(engs[c], corpora[f], lens, args.batch)
                rates.setdefault((f, c), []).append(rate)
                print("f = %-6.4g %-14s %8.0f issue reports/s   rescored %d routed %d of %d" % (f, c, rate, resc, routed, args.rows), flush=True)
    for e in engs.values():
        e.close()

    mean = {k: float(np.mean(v)) for k, v in rates.items()}
    spread = {k: float(np.max(v) - np.min(v)) for k, v in rates.items()}
    print()
    for k in sorted(rates, key=lambda k: (k[0], k[1])):
        print("f = %-6.4g %-14s %s mean %.0f spread %.0f" % (k[0], k[1], [round(x) for x in rates[k]], mean[k], spread[k]))
    print()
    print("%-8s %10s %10s %10s   %s" % ("f", "guarded", "routed", "safe", "time per report relative to guarded at f = 0: measured guarded / routed / safe | model 1 + 1.34 f / 1 + 0.34 f / 1.34"))
    t0 = 1.0 / mean[(0.0, "guarded")]
    for f in SHARES:
        g, r, s = (mean[(f, c)] for c in CONFIGS)
        print("%-8.4g %10.0f %10.0f %10.0f   %.3f / %.3f / %.3f | %.3f / %.3f / %.3f" % (f, g, r, s, 1 / g / t0, 1 / r / t0, 1 / s / t0, 1 + 1.34 * f, 1 + 0.34 * f, 1.34))
    print()
    if args.parent_tree:
        p, sp = mean[(0.0, "parent guarded")], spread[(0.0, "parent guarded")]
        d = mean[(0.0, "routed")] - p
        print("A. f = 0: routed %.0f against the parent's guarded form %.0f (spread %.0f): %+.0f -> %s" % (mean[(0.0, "routed")], p, sp, d, "within the spread" if abs(d) <= sp else
              ("ABOVE the spread" if d > 0 else "BELOW the spread: a finding")))
    for f in SHARES:
        g, r = mean[(f, "guarded")], mean[(f, "routed")]
        sp = max(spread[(f, "guarded")], spread[(f, "routed")])
        print("B. f = %-6.4g routed %.0f against guarded %.0f (spread %.0f): %+.0f -> %s" % (f, r, g, sp, r - g, "not slower" if r >= g - sp else "SLOWER beyond the spread: a finding"))


if __name__ == "__main__":
    main()
