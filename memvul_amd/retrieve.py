"""Per-anchor retrieval over a kept corpus: which issue reports does an anchor attract?  ctypes binding of libmemvul_retrieve.so (include/memvul_retrieve.h;
kernels: csrc/report_topk.h) and its command line.

The engine answers "which anchors fit this report"; a ReportIndex answers the other direction: for every query vector — an anchor of the bank, or
``engine.encode(...)`` of a fresh CVE description — the k rows of the corpus with the highest P(same), ranked ``(P descending, row ascending)`` on the GPU.  P(same) of
a pair is bit for bit what the engine's matcher gives for it.  As everywhere in this package there is no CPU fallback.

  python -m memvul_amd.retrieve --archive A --golden G --input T --k 20 [--anchors CWE-79,CWE-89] [--out FILE]

writes one JSON line per anchor: {"anchor": label, "reports": [{"Issue_Url", "row", "prob"}, ...]}."""
from __future__ import annotations

import ctypes as C
import os
import sys
from typing import Optional

import numpy as np

from .kept_index import KeptIndex, _check_array, _int, _ptr, load_side_library  # noqa: F401  (the kept-corpus index the four libraries share)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libmemvul_retrieve.so")

MAX_K, MAX_QUERIES, MAX_ROWS, MAX_PSAME = 64, 4096, 2 ** 31 - 2, 2 ** 28  # include/memvul_retrieve.h

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
    from . import kept_sweep as front

    ap = front.parser("python -m memvul_amd.retrieve", "For every anchor of the golden file: the k issue reports it attracts most.")
    ap.add_argument("--k", type=int, default=20, help="reports per anchor (1 .. 64)")
    front.add_anchors(ap)
    front.add_output(ap, "JSON lines")
    args = ap.parse_args(argv)
    if not 1 <= args.k <= MAX_K:
        ap.error(f"--k {args.k}: 1 .. {MAX_K}")
    corpus = front.read_corpus(ap, args)
    with front.filled_index(corpus, args, ReportIndex, engine_factory, index_factory) as (index, v):
        p, rows = index.query(v, min(args.k, MAX_K))
    front.write_json(args.out, format_reports(corpus.wanted_labels, corpus.urls, p, rows))
    return 0


if __name__ == "__main__":
    sys.exit(main())
