"""What re-matching a resident corpus costs next to sweeping it again (include/memvul_hip.h mv_corpus_rematch).  Writes profiles/rematch_bench.txt.

The 12-layer random-init model of bench.py, 16 384 resident rows at S = 256, the default compute dtype, k = 10 kept; two bank sizes, 124 and 1 000, each then
grown by 8 anchors.  Three things are timed, wall clock between two mv_sync, three alternating repeats each:
    sweep     mv_corpus_run over all rows against the grown bank (the only way to score it without kept embeddings)
    full      mv_corpus_rematch(g_first = 0)
    appended  mv_corpus_rematch(g_first = the old anchor count), after the stored results were put back to the old bank (untimed)
and the ratios sweep / full and sweep / appended are printed with the repeat-to-repeat spread (max / min - 1) of each.

    python scripts/rematch_rate.py [--out profiles/rematch_bench.txt] [--baseline FILE]
    python scripts/rematch_rate.py --sweep-only      # the sweep alone, without keeping anything: runs on a checkout from before mv_corpus_keep, whose
                                                     # output, given as --baseline, is quoted next to this tree's sweep
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from memvul_amd import synth  # noqa: E402
from memvul_amd.binding import Engine  # noqa: E402

N, S, BATCH, K, GROW, REPEATS = 16384, 256, 256, 10, 8, 3
BANKS = (124, 1000)


def timed(eng, call):
    eng.sync()
    t0 = time.perf_counter()
    call()
    eng.sync()
    return (time.perf_counter() - t0) * 1e3


def spread(v):
    return max(v) / min(v) - 1.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rematch_bench.txt"))
    ap.add_argument("--baseline", default=None, help="the output of --sweep-only on the parent commit")
    ap.add_argument("--sweep-only", action="store_true")
    args = ap.parse_args()

    dims = synth.BertDims(layers=12)
    w = synth.make_weights(dims)
    ids, lens = synth.make_ids(N, S, dims.vocab_size)
    rng = np.random.default_rng(synth.SEED + 1008)
    bank = rng.standard_normal((max(BANKS) + GROW, 512)).astype(np.float32)
    eng = Engine(0, vocab_size=dims.vocab_size, layers=dims.layers, max_tokens=BATCH * S, max_batch=BATCH, max_anchors=1024)
    eng.load_state_dict(w)
    lines = [f"rematch_rate: {N} resident rows x {S} tokens, 12 layers, compute dtype precise (default), batch {BATCH}, k = {K if not args.sweep_only else 0} kept, "
             f"banks {BANKS} each grown by {GROW}; wall ms between two mv_sync, {REPEATS} alternating repeats"]

    def sweep():
        eng.corpus_run(0, N, BATCH)

    for G0 in BANKS:
        G1 = G0 + GROW
        eng.anchor_set(bank[:G0])
        eng.corpus_upload(ids, lens)
        if not args.sweep_only:
            eng.corpus_keep(True, K)
        timed(eng, sweep)  # warm-up, and the sweep whose results the bank then outgrows
        eng.anchor_set(bank[:G1])
        t = {"sweep": [], "full": [], "appended": []}
        for rep in range(REPEATS):
            t["sweep"].append(timed(eng, sweep))
            if args.sweep_only:
                continue
            t["full"].append(timed(eng, lambda: eng.corpus_rematch(0, N, 0)))
            eng.anchor_set(bank[:G0])  # the stored results back to the old bank (untimed)
            eng.corpus_rematch(0, N, 0)
            eng.anchor_set(bank[:G1])
            t["appended"].append(timed(eng, lambda: eng.corpus_rematch(0, N, G0)))
        for what in ("sweep", "full", "appended"):
            if t[what]:
                v = t[what]
                lines.append(f"G {G0:4d} -> {G1:4d}  {what:9s} ms " + " ".join(f"{x:10.3f}" for x in v) + f"   median {np.median(v):10.3f}   spread {spread(v):6.1%}")
        if not args.sweep_only:
            ms = {k: float(np.median(v)) for k, v in t.items()}
            lines.append(f"G {G0:4d} -> {G1:4d}  ratio sweep / full {ms['sweep'] / ms['full']:8.1f}x   sweep / appended {ms['sweep'] / ms['appended']:8.1f}x   "
                         f"full / appended {ms['full'] / ms['appended']:6.2f}x   ({N / ms['sweep'] * 1e3:.0f} rows/s swept, {N / ms['full'] * 1e3:.0f} rows/s re-matched in full, "
                         f"{N / ms['appended'] * 1e3:.0f} rows/s appended)")
    eng.close()
    if args.baseline:
        lines.append("the sweep alone on the parent commit (nothing kept; same script, --sweep-only):")
        lines += ["    " + ln.rstrip("\n") for ln in open(args.baseline) if ln.strip()]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if not args.sweep_only:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
