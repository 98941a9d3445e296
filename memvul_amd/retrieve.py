"""Per-anchor retrieval over a kept corpus: which issue reports does an anchor attract?  ctypes binding of libmemvul_retrieve.so (include/memvul_retrieve.h;
kernels: csrc/report_topk.h) and its command line.

The engine answers "which anchors fit this report"; a ReportIndex answers the other direction: for every query vector — an anchor of the bank, or
``engine.encode(...)`` of a fresh CVE description — the k rows of the corpus with the highest P(same), ranked ``(P descending, row ascending)`` on the GPU.  P(same) of
a pair is bit for bit what the engine's matcher gives for it.  As everywhere in this package there is no CPU fallback.

  python -m memvul_amd.retrieve --archive A --golden G --input T --k 20 [--anchors CWE-79,CWE-89] [--out FILE]

writes one JSON line per anchor: {"anchor": label, "reports": [{"Issue_Url", "row", "prob"}, ...]}."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
from typing import Optional

import numpy as np

from .kept_index import KeptIndex, _check_array, _int, _ptr, load_side_library  # noqa: F401  (the kept-corpus index the three libraries share)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libmemvul_retrieve.so")

MAX_K, MAX_QUERIES, MAX_ROWS, MAX_PSAME = 64, 4096, 2 ** 31 - 2, 2 ** 28  # include/memvul_retrieve.h
KEY_MATCH_W = "_projector.weight"

_f32p, _vp = C.POINTER(C.c_float), C.c_void_p
_SIGNATURES = {
    "mvr_create": (C.c_int, [C.c_int, C.c_int, _vp, C.c_int, C.POINTER(_vp)]),
    "mvr_destroy": (None, [_vp]),
    "mvr_last_error": (C.c_char_p, [_vp]),
    "mvr_add": (C.c_int, [_vp, _vp, C.c_int64]),
    "mvr_reset": (C.c_int, [_vp]),
    "mvr_count": (C.c_int64, [_vp]),
    "mvr_query": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int64, C.c_int64, _vp, _vp]),
    "mvr_psame": (C.c_int, [_vp, _vp, C.c_int, C.c_int64, C.c_int64, _vp]),
    "mvr_kernel_ms": (C.c_int, [_vp, _f32p]),
    "mvr_test_plan": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int]),
}
RETRIEVE_SYMBOLS = list(_SIGNATURES)


def load_library(path: Optional[str] = None):
    """dlopen libmemvul_retrieve.so and declare the prototypes.  Raises RuntimeError if it is missing: there is no other implementation to fall back to."""
    return load_side_library(path or LIB_PATH, "libmemvul_retrieve.so", _SIGNATURES, "per-anchor retrieval has no CPU fallback")


class ReportIndex(KeptIndex):
    """One index <-> one GPU <-> one stream; one thread uses it at a time.  ``matcher_weight``: ``_projector.weight`` of the state dict, fp32 [2, 3 * proj_dim]."""

    PREFIX, VECTORS, MAX_VECTORS, MAX_ROWS = "mvr_", "query vectors", MAX_QUERIES, MAX_ROWS
    _load = staticmethod(lambda: load_library())

    # -- the questions
    def query(self, vectors: np.ndarray, k: int, first: int = 0, count: Optional[int] = None):
        """For each of the Q vectors the k best rows among [first, first + count): ``(p float32 [Q, k], rows int64 [Q, k])``, ranked (P(same) descending, row
        ascending; a NaN ranks first).  Slots beyond the rows in range hold p = -1, row = -1."""
        h = self._handle()
        vectors = self._vectors(vectors)
        k = _int(k, "k")
        if not 1 <= k <= MAX_K:
            raise ValueError(f"k = {k}: 1 <= k <= {MAX_K}")
        first, count = self._range(first, count)
        Q = vectors.shape[0]
        p, rows = np.empty((Q, k), np.float32), np.empty((Q, k), np.int64)
        self._check(self._lib.mvr_query(h, _ptr(vectors), Q, k, first, count, _ptr(p), _ptr(rows)), "mvr_query")
        return p, rows

    def psame(self, vectors: np.ndarray, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """P(same) float32 [count, Q] of rows [first, first + count) against every vector (count * Q <= 2^28 per call)."""
        h = self._handle()
        vectors = self._vectors(vectors)
        first, count = self._range(first, count)
        Q = vectors.shape[0]
        if count * Q > MAX_PSAME:
            raise ValueError(f"count * Q = {count * Q}: at most 2^28 values per call")
        p = np.empty((count, Q), np.float32)
        self._check(self._lib.mvr_psame(h, _ptr(vectors), Q, first, count, _ptr(p)), "mvr_psame")
        return p

    def test_plan(self, block_rows: int = 0, fan_in: int = 0, anchor_group: int = 0):
        """Tests only: rows per block, lists per merge launch, query vectors per group (0 = the library's own choice).  No result depends on them."""
        self._check(self._lib.mvr_test_plan(self._handle(), int(block_rows), int(fan_in), int(anchor_group)), "mvr_test_plan")

def format_reports(labels, urls, p: np.ndarray, rows: np.ndarray, first: int = 0) -> list:
    """One entry per query vector: {"anchor": label, "reports": [{"Issue_Url", "row", "prob"}, ...]} (exhausted slots left out).  rows: row numbers of the index;
    ``first``: the row of ``urls`` that row 0 of the index is."""
    out = []
    for g, label in enumerate(labels):
        reports = [{"Issue_Url": urls[first + int(r)], "row": first + int(r), "prob": float(pp)} for pp, r in zip(p[g], rows[g]) if r >= 0]
        out.append({"anchor": label, "reports": reports})
    return out


# ---- the command line ------------------------------------------------------------------------------------------------------------------------------------------

def main(argv=None, engine_factory=None, index_factory=None) -> int:
    from . import audit as _audit
    from . import binding

    ap = argparse.ArgumentParser(prog="python -m memvul_amd.retrieve", description="For every anchor of the golden file: the k issue reports it attracts most.")
    ap.add_argument("--archive", required=True, help="model.tar.gz or its extracted directory")
    ap.add_argument("--golden", required=True, help="the golden anchor file ({cwe_id: description})")
    ap.add_argument("--input", required=True, help="the issue reports (a test_ / validation_ file of the reader)")
    ap.add_argument("--k", type=int, default=20, help="reports per anchor (1 .. 64)")
    ap.add_argument("--anchors", default=None, metavar="LABEL[,LABEL...]", help="only these anchors (default: all of the golden file)")
    ap.add_argument("--out", default=None, help="write the JSON lines here instead of standard output")
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    if not 1 <= args.k <= MAX_K:
        ap.error(f"--k {args.k}: 1 .. {MAX_K}")
    sd, config, same_idx = _audit._read_archive(args.archive)
    if config is None:
        ap.error("--archive must be an archive (config.json, vocabulary/, weights): the readers come from its config")
    from . import archive as _archive

    reader = _archive._build_reader(config.get("validation_dataset_reader")) or _archive._build_reader(config.get("dataset_reader"))
    labels = list(reader.read_dataset(args.golden).keys())
    ids, lens, aids, alens = _audit._read_inputs(config, args.golden, args.input)
    urls = reader.read_arrays(args.input)["urls"]
    wanted = list(range(len(labels)))
    if args.anchors is not None:
        names = [a for a in args.anchors.split(",") if a]
        missing = [a for a in names if a not in labels]
        if missing:
            ap.error("--anchors: not in the golden file: " + ",".join(missing))
        wanted = [labels.index(a) for a in names]
    opts = dict(max_tokens=128 * 512, max_batch=max(512, args.batch), max_anchors=max(1024, len(alens)), same_idx=same_idx)
    opts.update(_audit._engine_dims(sd))
    eng = (engine_factory or binding.Engine)(args.device, **opts)
    try:
        eng.load_state_dict(sd)
        for i in range(len(alens)):  # (every anchor at its own length, the bank in the file's order)
            eng.anchor_append(np.ascontiguousarray(aids[i:i + 1, :max(int(alens[i]), 1)]), np.ascontiguousarray(alens[i:i + 1]))
        eng.bucketed_sweep(ids[:, :max(int(lens.max()), 1)], lens, args.batch, keep=True)
        index = ReportIndex.from_sweep(eng, np.asarray(sd[KEY_MATCH_W], np.float32), same_idx, index_factory=index_factory)
        try:
            v = np.ascontiguousarray(eng.anchor_get()[wanted], dtype=np.float32)
            p, rows = index.query(v, min(args.k, MAX_K))
        finally:
            index.close()
    finally:
        eng.close()
    lines = [json.dumps(e) for e in format_reports([labels[i] for i in wanted], urls, p, rows)]
    if args.out:
        with open(args.out, "w") as f:
            f.write("".join(ln + "\n" for ln in lines))
    else:
        print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
