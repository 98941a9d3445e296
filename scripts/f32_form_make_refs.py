"""float64 logits of the 14 committed sink cases (tests/golden/r06_sink_refs.npz) — what the fp32 form (compute dtype "f32", include/memvul_hip.h MV_F32) is
held against at 3e-5 by tests/test_f32_form_gpu.py.  Computed ONCE on a CPU-only machine with the numpy oracle at dtype=np.float64 and committed as
tests/golden/f32_form_refs.npz (one float64 [8, 6, 2] array per case), so that the GPU box spends its minutes on the engine.

The cases are fed as tests/test_safe_form_gpu.py::_sink_logits_err feeds the engine: the anchors one at a time at their own length, the 8 issue reports as one
batch of 256 tokens.  20 - 60 s per case.
Usage: python scripts/f32_form_make_refs.py"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from memvul_amd import synth  # noqa: E402
from oracle import memvul_oracle as orc  # noqa: E402
import r06_make_sink_refs as mk6  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "f32_form_refs.npz")
SINK_REFS = os.path.join(ROOT, "tests", "golden", "r06_sink_refs.npz")
CASES = (["sep_all_80_3001", "sep_all_95_3001", "sep_cls_80_3002", "cls_all_80_3001", "sep_all_50_3003"]
         + [f"{cell}_{seed}" for cell in ("mid_all_50", "mid_all_80", "mid_cls_80") for seed in (3001, 3002, 3003)])


def sink_case(refs, case):
    """(dims, weights, ids, lens, aids, alens) of a committed sink case, rebuilt from its stored gains."""
    token, rows, pct, seed = case.split("_")
    return mk6.case(token, rows, int(pct) / 100.0, int(seed), gains=refs[case + "_gains"])[:6]


def logits64(w, ids, lens, aids, alens):
    v = np.concatenate([orc.instance_forward(w, aids[g:g + 1, :int(alens[g])].astype(np.int64), np.ones((1, int(alens[g])), bool), dtype=np.float64)
                        for g in range(len(alens))], 0)
    u = orc.instance_forward(w, ids.astype(np.int64), synth.mask_from_lens(lens, ids.shape[1]), dtype=np.float64)
    return orc.match(u, v, w[synth.KEY_MATCH_W])[0]


def main():
    refs = np.load(SINK_REFS)
    have = dict(np.load(OUT)) if os.path.exists(OUT) else {}
    for case in CASES:
        if case in have:
            continue
        t0 = time.time()
        dims, w, ids, lens, aids, alens = sink_case(refs, case)
        lg = logits64(w, ids, lens, aids, alens)
        assert lg.dtype == np.float64 and lg.shape == (8, 6, 2)
        have[case] = lg
        print("%s: max |logit| %.2f  committed fp32 reference - float64: %.2e  (%.0f s)" % (
            case, float(np.abs(lg).max()), float(np.abs(refs[case + "_lg"] - lg).max()), time.time() - t0), flush=True)
        np.savez_compressed(OUT, **have)


if __name__ == "__main__":
    main()
