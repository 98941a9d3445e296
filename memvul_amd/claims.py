"""Per-anchor claims over a kept corpus: which issue reports does an anchor claim at the decision threshold, and how broad is it at every threshold of a grid?
ctypes binding of libmemvul_claims.so (include/memvul_claims.h; kernels: csrc/claim_sweep.h) and its command line.

The reference decides by a threshold, not by a rank (predict_memory.py:170-177: ``prob >= thres``; custom_metric.py:35-52 finds the threshold on a grid).  A
ClaimIndex answers by that rule for every query vector — an anchor of the bank, or ``engine.encode(...)`` of a fresh CVE description:

  select   EVERY row of the corpus with P(same) >= the vector's threshold, compacted on the GPU (only the survivors cross PCIe);
  counts   per vector and threshold, the number of rows of class 0 and of class 1 it claims (the per-anchor form of find_best_thres; nothing but [Q, T, 2] comes back).

P(same) of a pair is bit for bit what the engine's matcher gives for it, and a NaN claims nothing.  As everywhere in this package there is no CPU fallback.

  python -m memvul_amd.claims --archive A --golden G --input T [--thres 0.5] [--grid reference|LO:HI:STEP] [--anchors CWE-79,CWE-89] [--counts-only] [--out FILE]

writes one JSON line per anchor: {"anchor", "thres", "claimed", "positives", "reports": [{"Issue_Url", "row", "prob"}, ...]} and, with --grid, "grid" and "best_thres"."""
from __future__ import annotations

import ctypes as C
import os
import sys
from typing import Optional

import numpy as np

from .kept_index import ClassedKeptIndex, _check_array, _int, _ptr, load_side_library  # noqa: F401  (the kept-corpus index the four libraries share)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libmemvul_claims.so")

MAX_THRESHOLDS, MAX_VECTORS, MAX_ROWS, MAX_PAIRS = 64, 4096, 2 ** 31 - 2, 2 ** 28  # include/memvul_claims.h
ERR_STATE = -5

_f32p, _vp = C.POINTER(C.c_float), C.c_void_p
_SIGNATURES = {
    "mvc_create": (C.c_int, [C.c_int, C.c_int, _vp, C.c_int, C.POINTER(_vp)]),
    "mvc_destroy": (None, [_vp]),
    "mvc_last_error": (C.c_char_p, [_vp]),
    "mvc_add": (C.c_int, [_vp, _vp, C.c_int64]),
    "mvc_reset": (C.c_int, [_vp]),
    "mvc_count": (C.c_int64, [_vp]),
    "mvc_set_classes": (C.c_int, [_vp, _vp, C.c_int64, C.c_int64]),
    "mvc_counts": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, C.c_int64, C.c_int64, _vp]),
    "mvc_select": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int64, C.c_int64, _vp]),
    "mvc_fetch": (C.c_int, [_vp, _vp, _vp]),
    "mvc_kernel_ms": (C.c_int, [_vp, _f32p]),
    "mvc_test_plan": (C.c_int, [_vp, C.c_int, C.c_int]),
}
CLAIMS_SYMBOLS = list(_SIGNATURES)


def load_library(path: Optional[str] = None):
    """dlopen libmemvul_claims.so and declare the prototypes.  Raises RuntimeError if it is missing: there is no other implementation to fall back to."""
    return load_side_library(path or LIB_PATH, "libmemvul_claims.so", _SIGNATURES, "per-anchor claims have no CPU fallback")


# ---- thresholds ---------------------------------------------------------------------------------------------------------------------------------------------------

def up32(t) -> np.ndarray:
    """The smallest fp32 >= t, elementwise, for float64 ``t``: then ``p32 >= up32(t)`` decides exactly as the reference's ``float(p32) >= t`` does (every fp32
    below up32(t) is below t, every fp32 at or above it is at or above t).  An fp32 value is its own up32.  Non-finite values are refused."""
    t = np.asarray(t, np.float64)
    if not np.isfinite(t).all():
        raise ValueError("a threshold is not finite")
    with np.errstate(over="ignore"):
        t32 = t.astype(np.float32)  # (round to nearest)
    t32 = np.where(t32.astype(np.float64) < t, np.nextafter(t32, np.float32(np.inf)), t32).astype(np.float32)
    if not np.isfinite(t32).all():
        raise ValueError("a threshold is beyond the range of fp32")
    return t32


def reference_grid() -> np.ndarray:
    """The 40 thresholds of the reference's sweep (custom_metric.py:38: ``np.arange(0.5, 0.9, 0.01)``), each rounded UP to fp32 — 0.51 is not an fp32 number."""
    return up32(np.arange(0.5, 0.9, 0.01))


def _thresholds(t, what: str) -> np.ndarray:
    """Thresholds as a contiguous fp32 array of the input's shape: fp32 arrays as they are, Python numbers and float64 rounded up (up32).  Nothing else is taken."""
    if isinstance(t, np.ndarray):
        if t.dtype == np.float32:
            if not np.isfinite(t).all():
                raise ValueError(f"{what}: a threshold is not finite")
            return t if t.flags["C_CONTIGUOUS"] else np.ascontiguousarray(t)  # (a 0-d array stays one)
        if t.dtype != np.float64:
            raise TypeError(f"{what}: float32 or float64, not {t.dtype}")
        return up32(np.ascontiguousarray(t) if t.ndim else t)
    if isinstance(t, (np.float32,)):
        return _thresholds(np.asarray(t), what)
    if isinstance(t, (list, tuple)):
        if not all(isinstance(x, (int, float, np.floating, np.integer)) and not isinstance(x, bool) for x in t):
            raise TypeError(f"{what}: numbers")
        if t and all(isinstance(x, np.float32) for x in t):
            return _thresholds(np.array(t, np.float32), what)
        return np.ascontiguousarray(up32(np.array([float(x) for x in t], np.float64)))
    if isinstance(t, bool) or not isinstance(t, (int, float, np.floating, np.integer)):
        raise TypeError(f"{what}: a number or an array of numbers, not {type(t).__name__}")
    return up32(float(t))


def order_by_prob(offsets: np.ndarray, rows: np.ndarray, p: np.ndarray):
    """Each vector's segment re-ordered (P descending, row ascending): the per-anchor top-k order (a selection holds no NaN)."""
    seg = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    order = np.lexsort((rows, -p.astype(np.float64), seg))
    return rows[order], p[order]


class ClaimIndex(ClassedKeptIndex):
    """One index <-> one GPU <-> one stream; one thread uses it at a time.  ``matcher_weight``: ``_projector.weight`` of the state dict, fp32 [2, 3 * proj_dim]."""

    PREFIX, MAX_VECTORS, MAX_ROWS = "mvc_", MAX_VECTORS, MAX_ROWS
    _load = staticmethod(lambda: load_library())

    # -- the questions
    def counts(self, vectors: np.ndarray, thresholds, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """int64 [Q, T, 2]: ``[q, t, c]`` = the rows of class c among [first, first + count) with P(row, q) >= thresholds[t].  1 <= T <= 64, in any order;
        Python floats and float64 are rounded up to fp32 (up32), fp32 values are taken as they are."""
        h = self._handle()
        vectors = self._vectors(vectors)
        if not isinstance(thresholds, (np.ndarray, list, tuple)):
            raise TypeError(f"thresholds: an array or a list, not {type(thresholds).__name__}")
        th = _thresholds(thresholds, "thresholds")
        if th.ndim != 1 or not 1 <= th.shape[0] <= MAX_THRESHOLDS:
            raise ValueError(f"thresholds of shape {list(th.shape)}: one dimension, 1 <= T <= {MAX_THRESHOLDS}")
        first, count = self._range(first, count)
        Q, T = vectors.shape[0], th.shape[0]
        out = np.empty((Q, T, 2), np.int64)
        self._check(self._lib.mvc_counts(h, _ptr(vectors), Q, _ptr(th), T, first, count, _ptr(out)), "mvc_counts")
        return out

    def select(self, vectors: np.ndarray, thres, first: int = 0, count: Optional[int] = None, order: str = "prob"):
        """Every row of [first, first + count) a vector claims: ``(offsets int64 [Q + 1], rows int64 [offsets[Q]], p float32 [offsets[Q]])`` — vector q's rows are
        ``rows[offsets[q]:offsets[q + 1]]``, each with its P(same).  thres: one threshold for all vectors or one per vector (rounded as in ``counts``).
        order="prob": each segment ranked (P descending, row ascending) on the host; order="row": ascending rows, as the library wrote them.  More than 2^28
        claimed pairs are refused."""
        h = self._handle()
        vectors = self._vectors(vectors)
        if order not in ("prob", "row"):
            raise ValueError(f"order = {order!r}: 'prob' or 'row'")
        Q = vectors.shape[0]
        th = _thresholds(thres, "thres")
        if th.ndim == 0:
            th = np.full((Q,), th, np.float32)
        if th.shape != (Q,):
            raise ValueError(f"thres of shape {list(th.shape)}: a number, or one per vector ({Q})")
        first, count = self._range(first, count)
        offsets = np.empty((Q + 1,), np.int64)
        self._check(self._lib.mvc_select(h, _ptr(vectors), Q, _ptr(th), first, count, _ptr(offsets)), "mvc_select")
        rows, p = self.fetch(int(offsets[Q]))
        if order == "prob":
            rows, p = order_by_prob(offsets, rows, p)
        return offsets, rows, p

    def fetch(self, total: int):
        """The held selection (``total`` = its offsets[Q]) in row order: ``(rows int64, p float32)``.  Raises unless a select was the last call on the index."""
        rows, p = np.empty((total,), np.int64), np.empty((total,), np.float32)
        self._check(self._lib.mvc_fetch(self._handle(), _ptr(rows), _ptr(p)), "mvc_fetch")
        return rows, p

    def test_plan(self, block_rows: int = 0, vector_group: int = 0):
        """Tests only: rows per block, vectors per group (0 = the library's own choice).  No result depends on them."""
        self._check(self._lib.mvc_test_plan(self._handle(), int(block_rows), int(vector_group)), "mvc_test_plan")


# ---- the per-anchor threshold rule and the output entries -----------------------------------------------------------------------------------------------------------

def best_threshold(thresholds, counts: np.ndarray, n_pos: int, n_neg: int):
    """find_best_thres (custom_metric.py:35-52) from one vector's counts [T, 2]: the threshold with the highest F1 of "claimed = predicted positive", thresholds
    visited in the given order, ``>=`` — the last one wins a tie, and an all-zero F1 column yields the last threshold.  Returns (thres, its metric dict)."""
    from .custom_metric import _prf

    best_f1, best = 0, None
    for t, (c0, c1) in zip(thresholds, np.asarray(counts).tolist()):
        m = _prf(c1, n_pos - c1, n_neg - c0, c0)
        if m["f1"] >= best_f1:
            best_f1, best = m["f1"], dict(m, thres=float(t))
    return (None, None) if best is None else (best["thres"], best)


def format_claims(labels, urls, thres, offsets, rows, p, positive, first: int = 0, grid=None, grid_counts=None, with_reports: bool = True) -> list:
    """One entry per vector: {"anchor", "thres", "claimed", "positives", "reports": [{"Issue_Url", "row", "prob"}, ...]}; with a grid also "grid":
    [{"thres", "claimed", "positives"}, ...] and "best_thres".  rows: row numbers of the index; ``first``: the row of ``urls`` that row 0 of the index is;
    positive: bool per row of the index; thres / grid: the thresholds as the caller gave them."""
    positive = np.asarray(positive, bool)
    n_pos = int(positive.sum())
    n_neg = int(positive.size) - n_pos
    out = []
    for g, label in enumerate(labels):
        r, pp = rows[offsets[g]:offsets[g + 1]], p[offsets[g]:offsets[g + 1]]
        e = {"anchor": label, "thres": float(thres[g]), "claimed": int(len(r)), "positives": int(positive[r].sum())}
        if with_reports:
            e["reports"] = [{"Issue_Url": urls[first + int(x)], "row": first + int(x), "prob": float(y)} for x, y in zip(r, pp)]
        if grid is not None:
            e["grid"] = [{"thres": float(t), "claimed": int(c0 + c1), "positives": int(c1)} for t, (c0, c1) in zip(grid, grid_counts[g].tolist())]
            e["best_thres"] = best_threshold(grid, grid_counts[g], n_pos, n_neg)[0]
        out.append(e)
    return out


def parse_grid(spec):
    """"reference" -> np.arange(0.5, 0.9, 0.01) (float64, as the reference spells it); "LO:HI:STEP" -> np.arange(LO, HI, STEP); a list is taken as it is."""
    if isinstance(spec, str):
        if spec == "reference":
            return np.arange(0.5, 0.9, 0.01)
        parts = spec.split(":")
        if len(parts) != 3:
            raise ValueError(f"grid {spec!r}: 'reference' or LO:HI:STEP")
        lo, hi, step = (float(x) for x in parts)
        if not step > 0 or not hi > lo:
            raise ValueError(f"grid {spec!r}: LO < HI and STEP > 0")
        spec = np.arange(lo, hi, step)
    grid = np.asarray(spec, np.float64)
    if grid.ndim != 1 or not 1 <= grid.shape[0] <= MAX_THRESHOLDS:
        raise ValueError(f"a grid of {grid.shape} thresholds: 1 .. {MAX_THRESHOLDS}")
    return grid


def claims_of(index, labels, urls, vectors, thres, positive, first: int = 0, grid=None, with_reports: bool = True) -> list:
    """The entries of format_claims for ``vectors`` over the whole of ``index``: one select at ``thres`` (a number or one per vector) and, with a grid, one counts."""
    Q = len(vectors)
    th = np.broadcast_to(np.asarray(thres, np.float64), (Q,)) if np.ndim(thres) == 0 else np.asarray(thres, np.float64)
    if th.shape != (Q,):
        raise ValueError(f"thres: a number, or one per vector ({Q}), not shape {list(th.shape)}")
    grid_counts = None
    if grid is not None:
        grid = parse_grid(grid)
        grid_counts = index.counts(vectors, grid)
    if with_reports:
        offsets, rows, p = index.select(vectors, np.ascontiguousarray(th), order="prob")
    else:  # claimed / positives at the vectors' own thresholds come from counts: thresholds in chunks of 64, the diagonal kept
        offsets, rows, p = np.zeros(Q + 1, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32)
    entries = format_claims(labels, urls, th, offsets, rows, p, positive, first, grid, grid_counts, with_reports)
    if not with_reports:
        uniq, inv = np.unique(th, return_inverse=True)
        for c0 in range(0, len(uniq), MAX_THRESHOLDS):
            cc = index.counts(vectors, np.ascontiguousarray(uniq[c0:c0 + MAX_THRESHOLDS]))
            for g in np.flatnonzero((inv >= c0) & (inv < c0 + MAX_THRESHOLDS)):
                entries[g]["claimed"], entries[g]["positives"] = int(cc[g, inv[g] - c0].sum()), int(cc[g, inv[g] - c0, 1])
    return entries


# ---- the command line ------------------------------------------------------------------------------------------------------------------------------------------

def main(argv=None, engine_factory=None, index_factory=None) -> int:
    from . import kept_sweep as front

    ap = front.parser("python -m memvul_amd.claims", "For every anchor of the golden file: the issue reports it claims at a threshold.")
    ap.add_argument("--thres", type=float, default=0.5, help="the decision threshold: a report is claimed when P(same) >= it")
    ap.add_argument("--grid", default=None, metavar="reference|LO:HI:STEP", help="also count the claims at every threshold of a grid and name the best by F1")
    front.add_anchors(ap)
    ap.add_argument("--counts-only", action="store_true", help="leave the reports out: counts alone")
    front.add_output(ap, "JSON lines")
    args = ap.parse_args(argv)
    if not np.isfinite(args.thres):
        ap.error(f"--thres {args.thres}: a finite number")
    grid = None
    if args.grid is not None:
        try:
            grid = parse_grid(args.grid)
        except ValueError as e:
            ap.error(f"--grid: {e}")
    corpus = front.read_corpus(ap, args)
    with front.filled_index(corpus, args, ClaimIndex, engine_factory, index_factory, corpus.positive) as (index, v):
        entries = claims_of(index, corpus.wanted_labels, corpus.urls, v, args.thres, corpus.positive, 0, grid, not args.counts_only)
    front.write_json(args.out, entries)
    return 0


if __name__ == "__main__":
    sys.exit(main())
