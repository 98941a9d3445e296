"""Per-anchor ranking quality over a kept corpus: how well does an anchor RANK the issue reports against their classes?  ctypes binding of libmemvul_rank.so
(include/memvul_rank.h; kernels: csrc/rank_sort.h) and its command line.

The reference judges the matcher by three numbers (custom_metric.py:86-90, predict_memory.py:148-154): the best threshold, ROC-AUC and average precision.  A
RankIndex gives them for every query vector — an anchor of the bank, or ``engine.encode(...)`` of a fresh CVE description — and for the bank as a whole (a report's
score = its maximum over the vectors, what the reference itself measures), from a sort per vector on the GPU: nothing but a few numbers per vector comes back.

  rank    per vector: (n_neg, n_pos, n_nan), u2 = twice the Mann-Whitney U (an exact integer; auc = u2 / (2 n_pos n_neg)), ap (sklearn's average_precision_score,
          float64) and the threshold that maximises F1 over EVERY distinct score, with (TP, FP) at it — fractions compared exactly, a tie to the highest threshold;
  curve   the whole curve of ONE ranking: per distinct score, descending, TP and FP at "claimed iff P >= score" — roc_curve(drop_intermediate=False) and
          precision_recall_curve, ready to plot.

P(same) of a pair is bit for bit what the engine's matcher gives for it; a row whose score is NaN is left out of the ranking and counted.  As everywhere in this
package there is no CPU fallback.

  python -m memvul_amd.rank --archive A --golden G --input T [--anchors CWE-79,CWE-89] [--no-bank] [--out FILE] [--thres-file-out FILE.json]
                            [--curve LABEL|bank --curve-out FILE]

writes one JSON line per anchor (and one for the bank): {"anchor", "n_pos", "n_neg", "n_nan", "auc", "ap", "best_thres", "best_f1", "best_claimed",
"best_positives"}; --thres-file-out writes {anchor: best_thres}, the file ``python -m memvul_amd.bank --thres-file`` reads."""
from __future__ import annotations

import ctypes as C
import json
import math
import os
import sys
from typing import Optional

import numpy as np

from .kept_index import ClassedKeptIndex, _check_array, _int, _ptr, load_side_library  # noqa: F401  (the Python base of the indexes over a kept corpus)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libmemvul_rank.so")

MAX_VECTORS, MAX_ROWS, MAX_RANK_ROWS = 4096, 2 ** 31 - 2, 1 << 26  # include/memvul_rank.h
ERR_STATE = -5

_f32p, _vp = C.POINTER(C.c_float), C.c_void_p
_SIGNATURES = {
    "mvk_create": (C.c_int, [C.c_int, C.c_int, _vp, C.c_int, C.POINTER(_vp)]),
    "mvk_destroy": (None, [_vp]),
    "mvk_last_error": (C.c_char_p, [_vp]),
    "mvk_add": (C.c_int, [_vp, _vp, C.c_int64]),
    "mvk_reset": (C.c_int, [_vp]),
    "mvk_count": (C.c_int64, [_vp]),
    "mvk_set_classes": (C.c_int, [_vp, _vp, C.c_int64, C.c_int64]),
    "mvk_rank": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int64, C.c_int64, _vp, _vp, _vp, _vp, _vp]),
    "mvk_curve": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int64, C.c_int64, C.POINTER(C.c_int64)]),
    "mvk_fetch": (C.c_int, [_vp, _vp, _vp, _vp]),
    "mvk_kernel_ms": (C.c_int, [_vp, _f32p]),
    "mvk_test_plan": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int64]),
}
RANK_SYMBOLS = list(_SIGNATURES)


def load_library(path: Optional[str] = None):
    """dlopen libmemvul_rank.so and declare the prototypes.  Raises RuntimeError if it is missing: there is no other implementation to fall back to."""
    return load_side_library(path or LIB_PATH, "libmemvul_rank.so", _SIGNATURES, "per-anchor ranking quality has no CPU fallback")


def _bool(x, what: str) -> bool:
    if not isinstance(x, (bool, np.bool_)):
        raise TypeError(f"{what}: True or False, not {type(x).__name__}")
    return bool(x)


def auc_of(u2: int, n_pos: int, n_neg: int):
    """u2 / (2 n_pos n_neg) by Python-int division (correctly rounded); None where a class is empty."""
    return None if n_pos == 0 or n_neg == 0 else int(u2) / (2 * int(n_pos) * int(n_neg))


class RankIndex(ClassedKeptIndex):
    """One index <-> one GPU <-> one stream; one thread uses it at a time.  ``matcher_weight``: ``_projector.weight`` of the state dict, fp32 [2, 3 * proj_dim].
    ``curve`` holds a curve on the device; ``fetch`` copies it as often as asked; every other call drops it."""

    PREFIX, MAX_VECTORS, MAX_ROWS = "mvk_", MAX_VECTORS, MAX_ROWS
    _load = staticmethod(lambda: load_library())

    def _dropped(self):
        self._points = None  # the size of the curve this object believes is held

    def _rank_range(self, first, count):
        first, count = self._range(first, count)
        if count > MAX_RANK_ROWS:
            raise ValueError(f"count = {count}: one call ranks at most {MAX_RANK_ROWS} rows")
        return first, count

    # -- the questions
    def rank(self, vectors: np.ndarray, first: int = 0, count: Optional[int] = None, bank: bool = False) -> dict:
        """The ranking quality of every vector over rows [first, first + count), and with ``bank`` one more slot for the maximum over the vectors: a dict of arrays
        with S = Q + bank entries — ``n`` int64 [S, 3] (n_neg, n_pos, n_nan), ``u2`` int64 [S], ``ap`` float64 [S] (NaN where there is no positive),
        ``best_thres`` float32 [S] (NaN likewise), ``best`` int64 [S, 2] (TP, FP at best_thres) — and ``auc``, a list of S Python floats, None where undefined."""
        h = self._handle()
        vectors = self._vectors(vectors)
        bank = _bool(bank, "bank")
        first, count = self._rank_range(first, count)
        Q = vectors.shape[0]
        S = Q + int(bank)
        out = dict(n=np.empty((S, 3), np.int64), u2=np.empty((S,), np.int64), ap=np.empty((S,), np.float64), best_thres=np.empty((S,), np.float32),
                   best=np.empty((S, 2), np.int64))
        self._dropped()
        self._check(self._lib.mvk_rank(h, _ptr(vectors), Q, int(bank), first, count, *(_ptr(out[k]) for k in ("n", "u2", "ap", "best_thres", "best"))), "mvk_rank")
        out["auc"] = [auc_of(u, n[1], n[0]) for u, n in zip(out["u2"].tolist(), out["n"].tolist())]
        return out

    def curve(self, vectors: np.ndarray, bank: bool = False, first: int = 0, count: Optional[int] = None):
        """The curve of ONE ranking — of the single vector, or with ``bank`` of the maximum over the vectors: ``(thres float32 [D] descending, tp int64 [D],
        fp int64 [D])``, one point per distinct score: the positives / negatives with P >= thres."""
        h = self._handle()
        vectors = self._vectors(vectors)
        bank = _bool(bank, "bank")
        if not bank and vectors.shape[0] != 1:
            raise ValueError(f"{vectors.shape[0]} vectors without bank=True: a curve is that of ONE ranking")
        first, count = self._rank_range(first, count)
        points = C.c_int64(-1)
        self._dropped()
        self._check(self._lib.mvk_curve(h, _ptr(vectors), vectors.shape[0], int(bank), first, count, C.byref(points)), "mvk_curve")
        self._points = int(points.value)
        return self.fetch()

    def fetch(self):
        """The held curve: ``(thres, tp, fp)``.  Raises unless a curve was the last call on the index."""
        self._handle()
        if self._points is None:
            raise RuntimeError("no curve is held: fetch follows curve, with no other call on the index in between")
        thres, tp, fp = np.empty((self._points,), np.float32), np.empty((self._points,), np.int64), np.empty((self._points,), np.int64)
        self._check(self._lib.mvk_fetch(self._handle(), _ptr(thres), _ptr(tp), _ptr(fp)), "mvk_fetch")
        return thres, tp, fp

    def stage_ms(self) -> dict:
        """HIP-event time of the last call's launches, in milliseconds: the whole and its three stages."""
        ms = (C.c_float * 4)()
        self._call("kernel_ms", C.cast(ms, _f32p))
        return dict(zip(("total", "score", "sort", "statistics"), (float(x) for x in ms)))

    def kernel_ms(self) -> float:
        """HIP-event time of the last call's launches, in milliseconds."""
        return self.stage_ms()["total"]

    def test_plan(self, tile_rows: int = 0, vector_group: int = 0, work_cap_bytes: int = 0):
        """Tests only: rows per sort tile, vectors per group, the workspace cap (0 = the library's own choice).  No result depends on them."""
        self._dropped()
        self._check(self._lib.mvk_test_plan(self._handle(), int(tile_rows), int(vector_group), int(work_cap_bytes)), "mvk_test_plan")


# ---- the output entries ------------------------------------------------------------------------------------------------------------------------------------------------

def format_ranking(labels, out: dict) -> list:
    """One entry per slot of ``rank``'s result: {"anchor", "n_pos", "n_neg", "n_nan", "auc", "ap", "best_thres", "best_f1", "best_claimed", "best_positives"};
    a slot beyond the labels is the bank's ("anchor": "bank").  auc / ap / best_thres / best_f1 are None where they are undefined."""
    S = len(out["u2"])
    if S not in (len(labels), len(labels) + 1):
        raise ValueError(f"{len(labels)} labels for {S} slots")
    entries = []
    for s in range(S):
        n_neg, n_pos, n_nan = (int(x) for x in out["n"][s])
        tp, fp = (int(x) for x in out["best"][s])
        ap, thres = float(out["ap"][s]), float(out["best_thres"][s])
        none = n_pos == 0
        entries.append({"anchor": labels[s] if s < len(labels) else "bank", "n_pos": n_pos, "n_neg": n_neg, "n_nan": n_nan, "auc": out["auc"][s],
                        "ap": None if none or math.isnan(ap) else ap, "best_thres": None if none else thres,
                        "best_f1": None if none else 2 * tp / (tp + fp + n_pos), "best_claimed": tp + fp, "best_positives": tp})
    return entries


def ranking_of(index, labels, vectors, bank: bool = True, first: int = 0, count=None) -> list:
    """The entries of format_ranking for ``vectors`` over rows [first, first + count) of ``index``: one rank call."""
    if len(labels) != len(vectors):
        raise ValueError(f"{len(labels)} labels for {len(vectors)} vectors")
    return format_ranking(list(labels), index.rank(vectors, first, count, bank=bank))


# ---- the command line --------------------------------------------------------------------------------------------------------------------------------------------------

def main(argv=None, engine_factory=None, index_factory=None) -> int:
    from . import kept_sweep as front

    ap = front.parser("python -m memvul_amd.rank", "For every anchor of the golden file: how well it ranks the issue reports (ROC-AUC, average precision, best-F1 cut).")
    front.add_anchors(ap)
    ap.add_argument("--no-bank", action="store_true", help="leave out the entry of the bank as a whole (a report's score = its maximum over the anchors)")
    ap.add_argument("--thres-file-out", default=None, metavar="FILE.json", help="write {anchor: best_thres}, the file `python -m memvul_amd.bank --thres-file` reads")
    ap.add_argument("--curve", default=None, metavar="LABEL|bank", help="also the whole curve of one anchor, or of the bank")
    ap.add_argument("--curve-out", default=None, metavar="FILE", help="where --curve writes {\"anchor\", \"thres\", \"tp\", \"fp\"}")
    front.add_output(ap, "JSON lines")
    args = ap.parse_args(argv)
    if (args.curve is None) != (args.curve_out is None):
        ap.error("--curve and --curve-out go together")
    corpus = front.read_corpus(ap, args)
    if args.curve is not None and args.curve != "bank" and args.curve not in corpus.wanted_labels:
        ap.error(f"--curve {args.curve}: not among the anchors")
    with front.filled_index(corpus, args, RankIndex, engine_factory, index_factory, corpus.positive) as (index, v):
        entries = ranking_of(index, corpus.wanted_labels, v, bank=not args.no_bank)
        curve = None
        if args.curve == "bank":
            curve = index.curve(v, bank=True)
        elif args.curve is not None:
            g = corpus.wanted_labels.index(args.curve)
            curve = index.curve(np.ascontiguousarray(v[g:g + 1]))
    front.write_json(args.out, entries)
    if args.thres_file_out:
        with open(args.thres_file_out, "w") as f:
            json.dump({e["anchor"]: e["best_thres"] for e in entries if e["anchor"] != "bank" and e["best_thres"] is not None}, f)
            f.write("\n")
    if curve is not None:
        with open(args.curve_out, "w") as f:
            json.dump({"anchor": args.curve, "thres": [float(x) for x in curve[0]], "tp": curve[1].tolist(), "fp": curve[2].tolist()}, f)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
