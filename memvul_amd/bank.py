"""The anchor-bank audit over a kept corpus: what does the bank decide AS A WHOLE once each anchor has its own threshold, which anchors earn their place, which
duplicate each other, and which candidate should be added?  ctypes binding of libmemvul_bank.so (include/memvul_bank.h; kernels: csrc/bank_cover.h) and its
command line.

A BankAudit scores the rows against the vectors once (``mark``) and keeps the marking B[q][n] = "vector q claims row n" (P(same) >= the vector's threshold, P(same)
bit for bit the engine's matcher's, a NaN claims nothing) on the GPU as a bit matrix.  Every question is then a population count over it, and only integers come back:

  totals        claimed[q][c]: rows of class c vector q claims
  multiplicity  m[n] = how many vectors claim row n -> hist[c][j] (hist[1][0]: the bank's false negatives; j >= 1: the union decision's TP / FP), and
                sole[q][c]: rows only q claims — exactly the TP and FP lost by deleting q
  overlap       overlap[q][r][c]: rows of class c both q and r claim
  greedy        a greedy cover by gain = w_pos * new positives - w_neg * new negatives, ties to the lowest index, ``fixed`` vectors covered from the start

As everywhere in this package there is no CPU fallback.

  python -m memvul_amd.bank --archive A --golden G --input T [--thres 0.5 | --thres-file FILE.json] [--top 20] [--w-pos 1] [--w-neg 1] [--max-rounds K] [--out FILE]

writes ONE JSON document: the dict of ``audit_of``."""
from __future__ import annotations

import ctypes as C
import json
import os
import sys
from typing import Optional

import numpy as np

from .claims import _thresholds, up32  # noqa: F401  (the same rule for thresholds: float64 rounded UP to fp32, fp32 taken as it is)
from .kept_index import ClassedKeptIndex, _check_array, _int, _ptr, load_side_library  # noqa: F401  (the kept-corpus index the four libraries share)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libmemvul_bank.so")

MAX_VECTORS, MAX_ROWS, MAX_WEIGHT, MAX_MARK_BYTES = 4096, 2 ** 31 - 2, 1 << 20, 4 << 30  # include/memvul_bank.h
ERR_STATE = -5

_f32p, _vp = C.POINTER(C.c_float), C.c_void_p
_SIGNATURES = {
    "mvb_create": (C.c_int, [C.c_int, C.c_int, _vp, C.c_int, C.POINTER(_vp)]),
    "mvb_destroy": (None, [_vp]),
    "mvb_last_error": (C.c_char_p, [_vp]),
    "mvb_add": (C.c_int, [_vp, _vp, C.c_int64]),
    "mvb_reset": (C.c_int, [_vp]),
    "mvb_count": (C.c_int64, [_vp]),
    "mvb_set_classes": (C.c_int, [_vp, _vp, C.c_int64, C.c_int64]),
    "mvb_mark": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int64, C.c_int64]),
    "mvb_totals": (C.c_int, [_vp, _vp]),
    "mvb_multiplicity": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "mvb_overlap": (C.c_int, [_vp, _vp]),
    "mvb_greedy": (C.c_int, [_vp, C.c_int64, C.c_int64, _vp, C.c_int, C.POINTER(C.c_int), _vp, _vp]),
    "mvb_kernel_ms": (C.c_int, [_vp, _f32p]),
    "mvb_test_plan": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int]),
}
BANK_SYMBOLS = list(_SIGNATURES)


def load_library(path: Optional[str] = None):
    """dlopen libmemvul_bank.so and declare the prototypes.  Raises RuntimeError if it is missing: there is no other implementation to fall back to."""
    return load_side_library(path or LIB_PATH, "libmemvul_bank.so", _SIGNATURES, "the anchor-bank audit has no CPU fallback")


def mark_bytes(Q: int, count: int) -> int:
    """What a held marking costs on the device: 8 bytes per vector and 64 rows (mvb_mark refuses more than MAX_MARK_BYTES before it allocates anything)."""
    return 8 * int(Q) * ((int(count) + 63) // 64)


class BankAudit(ClassedKeptIndex):
    """One index <-> one GPU <-> one stream; one thread uses it at a time.  ``matcher_weight``: ``_projector.weight`` of the state dict, fp32 [2, 3 * proj_dim].
    ``mark`` holds a marking; ``totals`` / ``multiplicity`` / ``overlap`` / ``greedy`` read it as often as asked; every other call drops it."""

    PREFIX, MAX_VECTORS, MAX_ROWS = "mvb_", MAX_VECTORS, MAX_ROWS
    _load = staticmethod(lambda: load_library())

    def _dropped(self):
        self._marked = None  # (Q, count) of the marking this object believes is held: sizes the output buffers

    # -- the marking
    def mark(self, vectors: np.ndarray, thres, first: int = 0, count: Optional[int] = None):
        """Score rows [first, first + count) against ``vectors`` (float32 [Q, proj_dim], 1 <= Q <= 4096) and hold the marking.  thres: one threshold for all vectors
        or one per vector; Python floats and float64 are rounded up to fp32 (claims.up32), fp32 values are taken as they are.  Returns (Q, count)."""
        h = self._handle()
        vectors = self._vectors(vectors)
        Q = vectors.shape[0]
        th = _thresholds(thres, "thres")
        if th.ndim == 0:
            th = np.full((Q,), th, np.float32)
        if th.shape != (Q,):
            raise ValueError(f"thres of shape {list(th.shape)}: a number, or one per vector ({Q})")
        first, count = self._range(first, count)
        if mark_bytes(Q, count) > MAX_MARK_BYTES:
            raise ValueError(f"the marking of {Q} vectors over {count} rows takes {mark_bytes(Q, count)} bytes: at most {MAX_MARK_BYTES} are held")
        self._marked = None
        self._check(self._lib.mvb_mark(h, _ptr(vectors), Q, _ptr(th), first, count), "mvb_mark")
        self._marked = (Q, count)
        return self._marked

    def _held(self, what: str):
        h = self._handle()
        if self._marked is None:
            raise RuntimeError(f"{what}: no marking is held — call mark(vectors, thres) first (add, reset, set_classes and test_plan drop it)")
        return h, self._marked[0], self._marked[1]

    def totals(self) -> np.ndarray:
        """int64 [Q, 2]: ``[q, c]`` = the rows of class c vector q claims."""
        h, Q, _ = self._held("totals")
        out = np.empty((Q, 2), np.int64)
        self._check(self._lib.mvb_totals(h, _ptr(out)), "mvb_totals")
        return out

    def multiplicity(self, per_row: bool = False):
        """``(hist int64 [2, Q + 1], sole int64 [Q, 2])``; with per_row also ``mult uint16 [count]`` (how many vectors claim the row) and ``sole_of int32 [count]``
        (the one claimant where there is exactly one, otherwise -1)."""
        h, Q, count = self._held("multiplicity")
        hist, sole = np.empty((2, Q + 1), np.int64), np.empty((Q, 2), np.int64)
        mult = np.empty((count,), np.uint16) if per_row else None
        sole_of = np.empty((count,), np.int32) if per_row else None
        self._check(self._lib.mvb_multiplicity(h, _ptr(hist), _ptr(sole), _ptr(mult) if per_row else None, _ptr(sole_of) if per_row else None), "mvb_multiplicity")
        return (hist, sole, mult, sole_of) if per_row else (hist, sole)

    def overlap(self) -> np.ndarray:
        """int64 [Q, Q, 2]: ``[q, r, c]`` = the rows of class c both q and r claim (symmetric; the diagonal is ``totals``)."""
        h, Q, _ = self._held("overlap")
        out = np.empty((Q, Q, 2), np.int64)
        self._check(self._lib.mvb_overlap(h, _ptr(out)), "mvb_overlap")
        return out

    def greedy(self, w_pos: int = 1, w_neg: int = 1, fixed=None, max_rounds: Optional[int] = None):
        """The greedy cover: ``(order int32 [rounds], gained int64 [rounds, 2])``, gained[i] = (new positives, new negatives) of pick i.  fixed: bool / uint8 [Q],
        the vectors that are covered from the start and never picked.  Weights: integers in 0 .. 2^20."""
        h, Q, _ = self._held("greedy")
        w_pos, w_neg = _int(w_pos, "w_pos"), _int(w_neg, "w_neg")
        for name, w in (("w_pos", w_pos), ("w_neg", w_neg)):
            if not 0 <= w <= MAX_WEIGHT:
                raise ValueError(f"{name} = {w}: 0 <= w <= 2^20")
        max_rounds = Q if max_rounds is None else _int(max_rounds, "max_rounds")
        if max_rounds < 0:
            raise ValueError(f"max_rounds = {max_rounds}")
        fx = None
        if fixed is not None:
            if not isinstance(fixed, np.ndarray) or fixed.dtype not in (np.dtype(np.uint8), np.dtype(bool)) or fixed.shape != (Q,):
                raise ValueError(f"fixed: a bool or uint8 array of {Q} entries")
            fx = np.ascontiguousarray(fixed).view(np.uint8)
        cap = min(max_rounds, Q)
        order, gained, rounds = np.full((max(cap, 1),), -1, np.int32), np.zeros((max(cap, 1), 2), np.int64), C.c_int(0)
        self._check(self._lib.mvb_greedy(h, w_pos, w_neg, _ptr(fx) if fx is not None else None, max_rounds, C.byref(rounds), _ptr(order), _ptr(gained)), "mvb_greedy")
        return order[:rounds.value].copy(), gained[:rounds.value].copy()

    def test_plan(self, block_rows: int = 0, vector_group: int = 0, word_chunk: int = 0):
        """Tests only: rows per block of the sweep, vectors per group, words per chunk (0 = the library's own choice).  No result depends on them."""
        self._marked = None
        self._check(self._lib.mvb_test_plan(self._handle(), int(block_rows), int(vector_group), int(word_chunk)), "mvb_test_plan")


# ---- the audit as one document ----------------------------------------------------------------------------------------------------------------------------------------

def _prf(tp: int, fp: int, fn: int) -> dict:
    precision = tp / (tp + fp) if tp + fp else 0.0
    recall = tp / (tp + fn) if tp + fn else 0.0
    f1 = 2 * precision * recall / (precision + recall) if precision + recall else 0.0
    return {"precision": precision, "recall": recall, "f1": f1}


def audit_of(labels, thres, n_pos: int, n_neg: int, totals, hist, sole, overlap, order=None, gained=None, top: int = 20, start=(0, 0), greedy_labels=None) -> dict:
    """The audit of a marking as one JSON-ready dict, from the library's integers alone.

    labels / thres: per vector of the marking; n_pos / n_neg: the rows of class 1 / 0 in the range; order / gained: a greedy cover over ``greedy_labels`` (default:
    the marking's own vectors) that began with ``start`` = (TP, FP) already covered.

      "union":    {"TP", "FP", "FN", "TN", "precision", "recall", "f1"}: a row is predicted positive when at least one vector claims it (hist, j >= 1)
      "anchors":  per vector {"anchor", "thres", "claimed": [neg, pos], "sole": [neg, pos], "f1_without"}: the union's F1 with that vector deleted
                  (TP - sole pos, FP - sole neg)
      "overlaps": the ``top`` pairs q < r by Jaccard of their claimed sets (|q and r| / |q or r|, pairs with an empty union left out; ties: by (q, r)), each
                  {"a", "b", "both": [neg, pos], "jaccard"}
      "greedy":   per pick {"anchor", "index", "new_pos", "new_neg", "TP", "FP"}: TP / FP cumulative, starting from what the fixed vectors cover"""
    totals, hist, sole = np.asarray(totals, np.int64), np.asarray(hist, np.int64), np.asarray(sole, np.int64)
    Q = len(labels)
    if totals.shape != (Q, 2) or hist.shape != (2, Q + 1) or sole.shape != (Q, 2):
        raise ValueError(f"audit_of(): {Q} labels, totals {list(totals.shape)}, hist {list(hist.shape)}, sole {list(sole.shape)}")
    th = np.broadcast_to(np.asarray(thres, np.float64), (Q,))
    if int(hist[1].sum()) != n_pos or int(hist[0].sum()) != n_neg:
        raise ValueError(f"audit_of(): the histogram counts {int(hist[1].sum())} / {int(hist[0].sum())} rows of class 1 / 0, not {n_pos} / {n_neg}")
    tp, fp = int(hist[1, 1:].sum()), int(hist[0, 1:].sum())
    fn, tn = int(hist[1, 0]), int(hist[0, 0])
    out = {"rows": n_pos + n_neg, "positives": n_pos, "union": dict(TP=tp, FP=fp, FN=fn, TN=tn, **_prf(tp, fp, fn)), "anchors": [], "overlaps": [], "greedy": []}
    for q in range(Q):
        s0, s1 = int(sole[q, 0]), int(sole[q, 1])
        out["anchors"].append({"anchor": labels[q], "thres": float(th[q]), "claimed": [int(totals[q, 0]), int(totals[q, 1])], "sole": [s0, s1],
                               "f1_without": _prf(tp - s1, fp - s0, fn + s1)["f1"]})
    if overlap is not None and top > 0:
        ov = np.asarray(overlap, np.int64)
        both = ov.sum(2)
        size = totals.sum(1)
        union = size[:, None] + size[None, :] - both
        qi, ri = np.triu_indices(Q, 1)
        keep = union[qi, ri] > 0
        qi, ri = qi[keep], ri[keep]
        jac = both[qi, ri] / union[qi, ri]
        for i in np.lexsort((ri, qi, -jac))[:top]:
            q, r = int(qi[i]), int(ri[i])
            out["overlaps"].append({"a": labels[q], "b": labels[r], "both": [int(ov[q, r, 0]), int(ov[q, r, 1])], "jaccard": float(jac[i])})
    if order is not None:
        names = labels if greedy_labels is None else greedy_labels
        ctp, cfp = int(start[0]), int(start[1])
        for q, (npos, nneg) in zip(np.asarray(order).tolist(), np.asarray(gained, np.int64).reshape(-1, 2).tolist()):
            ctp, cfp = ctp + npos, cfp + nneg
            out["greedy"].append({"anchor": names[q], "index": int(q), "new_pos": int(npos), "new_neg": int(nneg), "TP": ctp, "FP": cfp})
    return out


def run_audit(index, labels, vectors, thres, positive, candidates=None, candidate_labels=None, candidate_thres=None, w_pos: int = 1, w_neg: int = 1,
              max_rounds: Optional[int] = None, top: int = 20, first: int = 0, count: Optional[int] = None) -> dict:
    """The calls behind ``audit_of`` on a filled index.  Without candidates: one marking of the bank; its totals, multiplicity, overlap, and the greedy order in
    which the bank would be rebuilt from nothing.  With candidates (fp32 [K, P]): the bank is marked alone for the union / sole / overlap figures, then bank and
    candidates together with the bank ``fixed``, and "greedy" ranks the candidates by marginal gain beyond what the bank covers ("candidates" names them)."""
    positive = np.asarray(positive, bool)
    n_pos = int(positive.sum())
    n_neg = int(positive.size) - n_pos
    Q = len(vectors)
    th = np.ascontiguousarray(np.broadcast_to(np.asarray(thres, np.float64), (Q,)))
    index.mark(vectors, th, first, count)
    totals = index.totals()
    hist, sole = index.multiplicity()
    overlap = index.overlap() if top > 0 else None
    if candidates is None:
        order, gained = index.greedy(w_pos, w_neg, None, max_rounds)
        return audit_of(list(labels), th, n_pos, n_neg, totals, hist, sole, overlap, order, gained, top)
    candidates = np.ascontiguousarray(candidates, np.float32)
    K = len(candidates)
    if candidate_labels is None:
        candidate_labels = [f"candidate {i}" for i in range(K)]
    if len(candidate_labels) != K:
        raise ValueError(f"{len(candidate_labels)} labels for {K} candidates")
    cth = np.broadcast_to(np.asarray(th[0] if candidate_thres is None else candidate_thres, np.float64), (K,))
    both = np.ascontiguousarray(np.concatenate([np.ascontiguousarray(vectors, np.float32), candidates]))
    fixed = np.concatenate([np.ones(Q, np.uint8), np.zeros(K, np.uint8)])
    index.mark(both, np.ascontiguousarray(np.concatenate([th, cth])), first, count)
    ctot = index.totals()[Q:]
    order, gained = index.greedy(w_pos, w_neg, fixed, max_rounds)
    start = (int(hist[1, 1:].sum()), int(hist[0, 1:].sum()))  # what the bank covers: the candidates' gains count beyond it
    out = audit_of(list(labels), th, n_pos, n_neg, totals, hist, sole, overlap, np.asarray(order) - Q, gained, top, start, list(candidate_labels))
    out["candidates"] = [{"anchor": candidate_labels[i], "thres": float(cth[i]), "claimed": [int(ctot[i, 0]), int(ctot[i, 1])]} for i in range(K)]
    return out


# ---- the command line -------------------------------------------------------------------------------------------------------------------------------------------------

def main(argv=None, engine_factory=None, index_factory=None) -> int:
    from . import kept_sweep as front

    ap = front.parser("python -m memvul_amd.bank", "The anchor bank of the golden file as a whole: union decision, sole claims, overlaps, greedy order.")
    ap.add_argument("--thres", type=float, default=0.5, help="the decision threshold of every anchor")
    ap.add_argument("--thres-file", default=None, metavar="FILE.json", help="{anchor: threshold}: per-anchor thresholds (e.g. the best_thres of memvul_amd.claims); others keep --thres")
    ap.add_argument("--top", type=int, default=20, help="how many overlapping pairs to list")
    ap.add_argument("--w-pos", type=int, default=1)
    ap.add_argument("--w-neg", type=int, default=1)
    ap.add_argument("--max-rounds", type=int, default=None)
    front.add_output(ap, "JSON document")
    args = ap.parse_args(argv)
    if not np.isfinite(args.thres):
        ap.error(f"--thres {args.thres}: a finite number")
    for name, w in (("--w-pos", args.w_pos), ("--w-neg", args.w_neg)):
        if not 0 <= w <= MAX_WEIGHT:
            ap.error(f"{name} {w}: 0 .. 2^20")
    if args.top < 0 or (args.max_rounds is not None and args.max_rounds < 0):
        ap.error("--top and --max-rounds: not negative")
    corpus = front.read_corpus(ap, args)
    labels = corpus.labels
    thres = np.full(len(labels), args.thres, np.float64)
    if args.thres_file is not None:
        with open(args.thres_file) as f:
            per = json.load(f)
        missing = [a for a in per if a not in labels]
        if missing:
            ap.error("--thres-file: not in the golden file: " + ",".join(missing))
        for a, t in per.items():
            if not isinstance(t, (int, float)) or not np.isfinite(t):
                ap.error(f"--thres-file: {a}: a finite number")
            thres[labels.index(a)] = float(t)
    with front.filled_index(corpus, args, BankAudit, engine_factory, index_factory, corpus.positive) as (index, v):
        doc = run_audit(index, labels, v, thres, corpus.positive, w_pos=args.w_pos, w_neg=args.w_neg, max_rounds=args.max_rounds, top=args.top)
    front.write_json(args.out, [doc])
    return 0


if __name__ == "__main__":
    sys.exit(main())
