"""What the tests of per-anchor ranking quality share (memvul_amd/rank.py, include/memvul_rank.h; nothing here needs a GPU): the definitions in Python integers and
fractions straight from a numpy sort, and a numpy restatement of the kernel plan of csrc/rank_sort.h that takes seeded faults."""
import math
import os
import shutil
from fractions import Fraction

import numpy as np

from memvul_amd import build

import report_index_kit as rkit  # noqa: F401  (the fixture of the kept-corpus tests)

NAN_KEY = 0xFFFFFFFF
FAULTS = ("tie_win", "unstable", "tie_cut", "f1_low", "nan_ranked", "local_class", "first_dropped")


def llvm_tool(name: str) -> str:
    """A tool of the ROCm installation's LLVM (llvm-readelf), on the path or next to hipcc."""
    hipcc = os.path.realpath(build.hipcc_path())
    for c in (shutil.which(name), os.path.join(os.path.dirname(os.path.dirname(hipcc)), "llvm", "bin", name), os.path.join(os.path.dirname(hipcc), name)):
        if c and os.path.exists(c):
            return c
    raise RuntimeError(f"{name} of the ROCm installation not found next to hipcc")


def keys_of(p: np.ndarray, cls: np.ndarray) -> np.ndarray:
    """key = bits << 1 | class (uint32); a NaN: all ones."""
    p = np.ascontiguousarray(p, np.float32)
    k = (p.view(np.uint32).astype(np.uint64) << np.uint64(1) | np.asarray(cls, np.uint64)).astype(np.uint32)
    return np.where(np.isnan(p), np.uint32(NAN_KEY), k)


def _groups(p, cls):
    """The tie groups of one ranking, thresholds descending: (thres fp32 [D], tp_g, fp_g, TP_g, FP_g) as int64 arrays, and (n_neg, n_pos, n_nan)."""
    p, cls = np.asarray(p, np.float32), np.asarray(cls).astype(bool)
    live = ~np.isnan(p)
    pl, cl = p[live], cls[live]
    thres, inv = np.unique(pl, return_inverse=True)  # ascending
    D = len(thres)
    tp = np.bincount(inv, weights=cl, minlength=D).astype(np.int64)[::-1]
    fp = np.bincount(inv, weights=~cl, minlength=D).astype(np.int64)[::-1]
    return thres[::-1].copy(), tp, fp, np.cumsum(tp), np.cumsum(fp), (int((~cl).sum()), int(cl.sum()), int((~live).sum()))


def reference_rank(p, cls) -> dict:
    """One ranking by the definitions of include/memvul_rank.h: n = (n_neg, n_pos, n_nan), u2 (int), ap (a Fraction, None without positives), best_thres (np.float32,
    NaN without positives), best = (TP, FP); and what the fixture conditions ask: groups, mixed (tie groups holding both classes), f1_ties (other thresholds with the
    best F1), interior (the best cut claims neither nothing but its own group nor everything)."""
    thres, tp, fp, TP, FP, (n_neg, n_pos, n_nan) = _groups(p, cls)
    out = dict(n=(n_neg, n_pos, n_nan), groups=len(thres), mixed=int(((tp > 0) & (fp > 0)).sum()))
    if n_pos == 0:
        return dict(out, u2=0, ap=None, best_thres=np.float32("nan"), best=(0, 0), f1_ties=0, interior=False)
    tp, fp, TP, FP = tp.tolist(), fp.tolist(), TP.tolist(), FP.tolist()  # Python integers from here on
    u2 = sum(a * (2 * (n_neg - F) + b) for a, b, F in zip(tp, fp, FP))
    # ap = sum tp_g TP_g / (n_pos (TP_g + FP_g)), exactly: over the common denominator of the groups that hold a positive
    L = math.lcm(*[T + F for a, T, F in zip(tp, TP, FP) if a])
    ap = Fraction(sum(a * T * (L // (T + F)) for a, T, F in zip(tp, TP, FP) if a), n_pos * L)
    g, ties = 0, 0  # F1_g = 2 TP_g / (TP_g + FP_g + n_pos), compared by cross products; thresholds descend: the first of equals is the highest
    for i in range(1, len(TP)):
        l, r = TP[i] * (TP[g] + FP[g] + n_pos), TP[g] * (TP[i] + FP[i] + n_pos)
        if l > r:
            g, ties = i, 0
        elif l == r:
            ties += 1
    return dict(out, u2=u2, ap=ap, best_thres=thres[g], best=(TP[g], FP[g]), f1_ties=ties, interior=0 < g < len(thres) - 1)


def reference_curve(p, cls):
    """(thres fp32 [D] descending, TP int64 [D], FP int64 [D])."""
    thres, _, _, TP, FP, _ = _groups(p, cls)
    return thres, TP.astype(np.int64), FP.astype(np.int64)


def bank_scores(ps: np.ndarray) -> np.ndarray:
    """The bank slot's score per row: the maximum over the vectors, NaN where any is."""
    ps = np.asarray(ps, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(ps).any(1), np.float32("nan"), ps.max(1)).astype(np.float32)


def reference_matrix(ps: np.ndarray, cls, bank: bool = False) -> dict:
    """reference_rank of every column (and of bank_scores) in the arrays RankIndex.rank returns, plus ``exact`` (the list of reference_rank dicts)."""
    cols = [ps[:, q] for q in range(ps.shape[1])] + ([bank_scores(ps)] if bank else [])
    exact = [reference_rank(c, cls) for c in cols]
    return dict(n=np.array([e["n"] for e in exact], np.int64).reshape(-1, 3), u2=np.array([e["u2"] for e in exact], np.int64),
                best_thres=np.array([e["best_thres"] for e in exact], np.float32), best=np.array([e["best"] for e in exact], np.int64).reshape(-1, 2), exact=exact)


def ap_bound(e: dict) -> Fraction:
    """(D + 3) 2^-53: D non-negative terms of at most three roundings each and D - 1 additions, the sum at most 1."""
    return Fraction(e["groups"] + 3, 2 ** 53)


# ---- the kernel plan in numpy ------------------------------------------------------------------------------------------------------------------------------------------

def plan_sort(keys: np.ndarray, tile: int, fault=None) -> np.ndarray:
    """Four passes of eight bits: per-tile digit histograms, an exclusive scan over (digit, tile), a stable scatter with the ranks formed inside the tile."""
    n = len(keys)
    ntiles = (n + tile - 1) // tile
    for shift in (0, 8, 16, 24):
        d = ((keys >> np.uint32(shift)) & np.uint32(255)).astype(np.int64)
        hist = np.zeros((ntiles, 256), np.int64)
        for t in range(ntiles):
            hist[t] = np.bincount(d[t * tile:(t + 1) * tile], minlength=256)
        off = np.cumsum(hist.T.reshape(-1)) - hist.T.reshape(-1)  # digits outermost
        off = off.reshape(256, ntiles).T
        out = np.empty_like(keys)
        for t in range(ntiles):
            dt = d[t * tile:(t + 1) * tile]
            order = np.argsort(dt, kind="stable")
            rank = np.empty(len(dt), np.int64)
            starts = np.cumsum(hist[t]) - hist[t]
            rank[order] = np.arange(len(dt)) - starts[dt[order]]  # same-digit keys at lower places of the tile
            if fault == "unstable":
                rank = hist[t][dt] - 1 - rank
            out[off[t][dt] + rank] = keys[t * tile:(t + 1) * tile]
        keys = out
    return keys


def _ap_fixed_shape(terms: np.ndarray) -> float:
    """float64 terms per position (0 where no group ends) summed as the kernels do: 64 by a butterfly, four such per 256, the 256-blocks strided over 256
    accumulators, those by a halving tree."""
    n = len(terms)
    nchunks = (n + 255) // 256
    x = np.zeros(nchunks * 256, np.float64)
    x[:n] = terms
    x = x.reshape(-1, 64)
    for m in (32, 16, 8, 4, 2, 1):
        x = x + x[:, np.arange(64) ^ m]
    w = x[:, 0].reshape(nchunks, 4)
    chunks = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    acc = np.zeros(256, np.float64)
    for c0 in range(0, nchunks, 256):
        part = chunks[c0:c0 + 256]
        acc[:len(part)] += part
    half = 128
    while half >= 1:
        acc[:half] = acc[:half] + acc[half:2 * half]
        half //= 2
    return float(acc[0])


def plan_rank(p_all: np.ndarray, cls_all: np.ndarray, first: int, count: int, tile: int, fault=None) -> dict:
    """One ranking over rows [first, first + count) of (p_all, cls_all) by the plan of csrc/rank_sort.h: keys, the sort, the class prefix, the group starts
    propagated over the tiles, the group ends, the reductions.  Returns the fields of reference_rank that the library returns, ap as a float."""
    p = np.asarray(p_all, np.float32)[first:first + count]
    rows = np.arange(count)
    if fault == "first_dropped":
        cls = np.asarray(cls_all)[rows]
    elif fault == "local_class":
        cls = np.asarray(cls_all)[first + rows % 256]
    else:
        cls = np.asarray(cls_all)[first + rows]
    keys = keys_of(p, cls)
    if fault == "nan_ranked":
        keys = (np.ascontiguousarray(p).view(np.uint32).astype(np.uint64) << np.uint64(1) | cls.astype(np.uint64)).astype(np.uint32)  # (0xff800000 | class: not the sentinel)
    if count == 0:
        return dict(n=(0, 0, 0), u2=0, ap=float("nan"), best_thres=np.float32("nan"), best=(0, 0))
    keys = plan_sort(keys, tile, fault)
    live = keys != np.uint32(NAN_KEY)
    M = int(live.sum())
    score = keys >> np.uint32(1)
    c = (live & ((keys & np.uint32(1)) == 1)).astype(np.int64)
    pos = np.arange(count)
    start = live & ((pos == 0) | (np.concatenate([[0], score[:-1]]) != score))
    end = live & (np.concatenate([score[1:], [NAN_KEY >> 1]]) != score)
    cpos = np.cumsum(c)
    ex = cpos - c
    # the last group start at or below each position, tile by tile with a carry
    ntiles = (count + tile - 1) // tile
    S, below = np.zeros(count, np.int64), np.zeros(count, np.int64)
    carry = (-1, 0)
    for t in range(ntiles):
        a, b = t * tile, min((t + 1) * tile, count)
        if fault == "tie_cut":
            carry = (a, int(ex[a]))  # "the tile's first row"
        last = np.maximum.accumulate(np.where(start[a:b], np.arange(a, b), -1))
        S[a:b] = np.where(last >= 0, last, carry[0])
        below[a:b] = np.where(last >= 0, ex[np.maximum(last, 0)], carry[1])
        if last[-1] >= 0:
            carry = (int(last[-1]), int(ex[last[-1]]))
    n_pos = int(c.sum())
    n_neg = M - n_pos
    if n_pos == 0:
        return dict(n=(n_neg, 0, count - M), u2=0, ap=float("nan"), best_thres=np.float32("nan"), best=(0, 0))
    e = np.flatnonzero(end)
    tp_g, TP = cpos[e] - below[e], n_pos - below[e]
    fp_g, FP = (e - S[e] + 1) - tp_g, (M - S[e]) - TP
    u2 = sum(int(a) * (2 * (n_neg - int(F)) + (2 if fault == "tie_win" else 1) * int(b)) for a, b, F in zip(tp_g, fp_g, FP))
    terms = np.zeros(count, np.float64)
    terms[e] = (tp_g.astype(np.float64) / np.float64(n_pos)) * (TP.astype(np.float64) / (TP + FP).astype(np.float64))
    best = None
    for i in range(len(e)):  # ascending thresholds; exact fractions
        f = Fraction(2 * int(TP[i]), int(TP[i]) + int(FP[i]) + n_pos)
        if best is None or f > best[0] or (f == best[0] and fault != "f1_low"):
            best = (f, i)
    g = best[1]
    return dict(n=(n_neg, n_pos, count - M), u2=u2, ap=_ap_fixed_shape(terms), best_thres=(score[e[g]]).astype(np.uint32).view(np.float32), best=(int(TP[g]), int(FP[g])))
