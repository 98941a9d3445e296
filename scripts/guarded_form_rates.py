"""Rate of the three forms of MV_F16X8 against the share of sequences that carry an ordinary-token attention sink (GPU).

A resident corpus of 256-token issue reports on the sink model mid_all_80_3001 (gains from tests/golden/r06_sink_refs.npz), swept in batches of 256, with the
share f of the rows marked with the sink token (synth.MID_ID at len // 2) and every other occurrence of that token replaced; the bank is the case's six marked
anchors.  Per (f, form): issue reports/s of the best of --repeat timed sweeps (corpus_run + corpus_results: the guarded form's rescoring is inside), and how
many rows were rescored.  The model: guarded = t_default (1 + 1.34 f).
Usage: python scripts/guarded_form_rates.py [--rows 4096] [--repeat 3]"""
import argparse
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from memvul_amd import synth  # noqa: E402
from memvul_amd.binding import Engine  # noqa: E402
import r06_make_sink_refs as mk6  # noqa: E402

SHARES = (0.0, 1 / 16, 1 / 4, 1.0)
FORMS = ("default", "guarded", "safe")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    refs = np.load(os.path.join(ROOT, "tests", "golden", "r06_sink_refs.npz"))
    dims, w, _, _, aids, alens = mk6.case("mid", "all", 0.8, 3001, gains=refs["mid_all_80_3001_gains"])[:6]
    n, S = args.rows, 256
    base, lens = synth.make_ids(n, S, dims.vocab_size, seed=synth.SEED + 31, ragged=False)
    base[base == synth.MID_ID] = synth.MID_ID + 1
    eng = Engine(0, vocab_size=dims.vocab_size, layers=12, max_tokens=args.batch * S, max_batch=args.batch, max_anchors=16)
    warnings.simplefilter("ignore")  # (the default form warns about the sink, the guarded form about the share: both are what is measured here)
    eng.load_state_dict(w, "precise")
    rate = {}
    for f in SHARES:
        ids = base.copy()
        marked = np.arange(n)[np.arange(n) % 16 < round(16 * f)]  # the same share in every batch
        if len(marked):
            ids[marked] = synth.mark_mid_token(ids[marked], lens[marked])
        for form in FORMS:
            eng.set_form(form)
            eng.anchor_reset()
            for g in range(len(alens)):
                eng.anchor_append(aids[g:g + 1, :int(alens[g])], alens[g:g + 1])
            eng.corpus_upload(ids, lens)
            best_t = None
            for it in range(args.repeat + 1):  # (the first sweep warms up)
                eng.form_stats(reset=True)
                eng.sync()
                t0 = time.perf_counter()
                eng.corpus_run(0, n, args.batch)
                eng.corpus_results(0, n)
                t = time.perf_counter() - t0
                if it:
                    best_t = t if best_t is None else min(best_t, t)
            seqs, resc = eng.form_stats()
            rate[(f, form)] = n / best_t
            print("f = %-6.4g %-8s %8.0f issue reports/s   rescored %d of %d" % (f, form, n / best_t, resc, seqs), flush=True)
    print()
    print("%-8s %10s %10s %10s %14s %12s" % ("f", "default", "guarded", "safe", "model guarded", "guarded/safe"))
    for f in SHARES:
        d, g, s = (rate[(f, k)] for k in FORMS)
        print("%-8.4g %10.0f %10.0f %10.0f %14.0f %12.2f" % (f, d, g, s, d / (1 + 1.34 * f), g / s))
    eng.close()


if __name__ == "__main__":
    main()
