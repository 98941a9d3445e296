"""CPU references for the GUARDED form of MV_F16X8 (include/memvul_hip.h mv_set_form; tests/test_guarded_form_gpu.py): batches in which only SOME sequences
carry an ordinary-token attention sink, so that the per-sequence choice between the default and the safe form has something to choose.

For three committed sink cases of tests/golden/r06_sink_refs.npz (scripts/r06_make_sink_refs.py; the gains are taken from there, nothing is calibrated again)
the case's 8 issue reports + the same 8 with every synth.MID_ID — the sink token — replaced by MID_ID + 1 (16 rows), against its 6 anchors + the same 6 unmarked
(12 anchors).  Stored per case: the fp32 reference logits [16, 12, 2] (oracle/hf_reference.py: HF BertModel fp32 + the reference's head).
Usage: python scripts/make_guarded_form_refs.py"""
import os
import sys

import numpy as np
import torch  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from memvul_amd import synth  # noqa: E402
import r05_make_refs as mk  # noqa: E402
import r06_make_sink_refs as mk6  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "guarded_form_refs.npz")
SINK_REFS = os.path.join(ROOT, "tests", "golden", "r06_sink_refs.npz")
CASES = ("mid_all_80_3001", "mid_all_50_3002", "mid_cls_80_3003")


def unmark(ids):
    """ids with every occurrence of the sink token replaced by its neighbour in the vocabulary: the same sequences without the sink."""
    ids = np.array(ids, copy=True)
    ids[ids == synth.MID_ID] = synth.MID_ID + 1
    return ids


def mixed_case(name, sink_refs):
    """(dims, weights, ids [16, 256], lens, aids [12, 512], alens, marked_rows, marked_anchors) of one case: rows 0 .. 7 / anchors 0 .. 5 carry the sink."""
    token, rows, pct, seed = name.split("_")
    dims, w, ids, lens, aids, alens = mk6.case(token, rows, int(pct) / 100.0, int(seed), gains=sink_refs[name + "_gains"])[:6]
    return (dims, w, np.concatenate([ids, unmark(ids)]), np.concatenate([lens, lens]), np.concatenate([aids, unmark(aids)]), np.concatenate([alens, alens]),
            np.arange(len(lens)), np.arange(len(alens)))


def main():
    sink_refs = np.load(SINK_REFS)
    have = dict(np.load(OUT)) if os.path.exists(OUT) else {}
    for name in CASES:
        if name + "_lg" in have:
            continue
        dims, w, ids, lens, aids, alens = mixed_case(name, sink_refs)[:6]
        lg = mk.reference(w, dims, ids, lens, aids, alens)[2]
        have[name + "_lg"] = lg
        print("%s: reference logits %s, max |logit| %.2f" % (name, lg.shape, float(np.abs(lg).max())), flush=True)
        np.savez_compressed(OUT, **have)


if __name__ == "__main__":
    main()
