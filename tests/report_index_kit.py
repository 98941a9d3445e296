"""Shared by the per-anchor retrieval tests (memvul_amd/retrieve.py, csrc/report_topk.h): the order in numpy, a numpy restatement of the kernel plan, and a tie-heavy
fixture.  Tests only."""
import numpy as np

NOROW = 0x7FFFFFFF


def key_of(p: np.ndarray) -> np.ndarray:
    """The rank key of report_topk.h rt_key: NaN -> 2.0 (above every probability)."""
    p = np.asarray(p, np.float32)
    return np.where(np.isnan(p), np.float32(2.0), p)


def reference_topk(p: np.ndarray, k: int, first: int = 0):
    """p [N, Q] -> (top_p float32 [Q, k], rows int64 [Q, k]): per column the order (key descending, row ascending); exhausted slots p = -1, row = -1.  The p handed
    back are the input's own bits (a NaN keeps its payload).  first: the row number of p[0]."""
    p = np.asarray(p, np.float32)
    N, Q = p.shape
    top_p, rows = np.full((Q, k), -1.0, np.float32), np.full((Q, k), -1, np.int64)
    key = key_of(p)
    for g in range(Q):
        order = np.lexsort((np.arange(N), -key[:, g].astype(np.float64)))[:k]
        top_p[g, :len(order)] = p[order, g]
        rows[g, :len(order)] = order + first
    return top_p, rows


def _select(p: np.ndarray, rows: np.ndarray, k: int, higher_row_wins: bool = False):
    """k rounds of arg-max over candidates (p, row); row NOROW = an exhausted slot.  Returns the list [k] of (p, row), exhausted entries (-1, NOROW)."""
    live = rows != NOROW
    p, rows = p[live], rows[live]
    order = np.lexsort((-rows if higher_row_wins else rows, -key_of(p).astype(np.float64)))[:k]
    out_p, out_r = np.full(k, -1.0, np.float32), np.full(k, NOROW, np.int64)
    out_p[:len(order)], out_r[:len(order)] = p[order], rows[order]
    return out_p, out_r


def plan_model(p: np.ndarray, k: int, block_rows: int, fan_in: int, anchor_group: int, fault: str = None):
    """The plan of report_topk.h on a P(same) matrix p [N, Q]: query vectors in groups of anchor_group; per group one list of k per block of block_rows rows (the
    block's k best), then merges of fan_in lists into one until one is left (at least one merge: it writes the result).  Returns what reference_topk returns.
    fault: one seeded defect — "tie_high" (ties broken by the higher row), "short_list" (a block's list truncated to k - 1), "drop_last" (a merge drops its last
    input list), "no_offset" (the row offset of the second block is not added)."""
    p = np.asarray(p, np.float32)
    N, Q = p.shape
    top_p, top_r = np.full((Q, k), -1.0, np.float32), np.full((Q, k), -1, np.int64)
    if N == 0:
        return top_p, top_r
    nblocks = (N + block_rows - 1) // block_rows
    for q0 in range(0, Q, anchor_group):
        for g in range(q0, min(q0 + anchor_group, Q)):
            lists = []
            for b in range(nblocks):
                r0 = b * block_rows
                rows = np.arange(r0, min(r0 + block_rows, N), dtype=np.int64)
                lp, lr = _select(p[rows, g], rows, k, higher_row_wins=fault == "tie_high")
                if fault == "no_offset" and b == 1:
                    lr = np.where(lr == NOROW, NOROW, lr - r0)
                if fault == "short_list":
                    lp[k - 1], lr[k - 1] = -1.0, NOROW
                lists.append((lp, lr))
            while True:
                out = []
                for l0 in range(0, len(lists), fan_in):
                    part = lists[l0:l0 + fan_in]
                    if fault == "drop_last" and len(part) > 1:
                        part = part[:-1]
                    out.append(_select(np.concatenate([x[0] for x in part]), np.concatenate([x[1] for x in part]), k, higher_row_wins=fault == "tie_high"))
                lists = out
                if len(lists) == 1:
                    break
            lp, lr = lists[0]
            top_p[g] = lp
            top_r[g] = np.where(lr == NOROW, -1, lr)
    return top_p, top_r


def merge_levels(n_rows: int, block_rows: int, fan_in: int) -> int:
    """Merge launches per group of query vectors."""
    lists, levels = (n_rows + block_rows - 1) // block_rows, 0
    while True:
        lists, levels = (lists + fan_in - 1) // fan_in, levels + 1
        if lists <= 1:
            return levels


def fixture(seed: int, N: int, P: int, Q: int, nan_row: int = None, block_rows: int = 64):
    """(U [N, P], V [Q, P], W_m [2, 3P]) fp32: non-negative embeddings with about half zeros (the header's output is a ReLU); exact duplicate rows placed in
    DIFFERENT blocks of block_rows rows (ties across lists) and next to each other (ties within one); duplicate query vectors; a matcher weight scaled so that
    |delta| spans about 0 .. 8 (P(same) neither all one half nor saturated); optionally one row holding a NaN."""
    rng = np.random.default_rng(seed)
    U = (np.maximum(rng.standard_normal((N, P)), 0) * rng.uniform(0.2, 1.5, (N, 1))).astype(np.float32)
    V = (np.maximum(rng.standard_normal((Q, P)), 0) * rng.uniform(0.2, 1.5, (Q, 1))).astype(np.float32)
    for a, b in ((0, block_rows), (1, 2 * block_rows + 3), (5, 4 * block_rows), (2, 3), (block_rows - 1, block_rows)):  # later copies of earlier rows
        if b < N and a < N:
            U[b] = U[a]
    if N > 8:
        U[N - 1] = U[N // 2]
    if Q > 2:
        V[Q - 1] = V[0]
    if Q > 4:
        V[3] = V[1]
    W = rng.uniform(-1.0, 1.0, (2, 3 * P)).astype(np.float32)
    # delta is a sum of ~P/2 terms of size ~|w| x ~0.8: scale so that its spread is a few units
    W *= np.float32(4.0 / (0.8 * np.sqrt(P)))
    if nan_row is not None and nan_row < N:
        U[nan_row, P // 3] = np.float32("nan")
    return np.ascontiguousarray(U), np.ascontiguousarray(V), np.ascontiguousarray(W)


def psame_f64(U, V, W, same_idx: int) -> np.ndarray:
    """P(same) [N, Q] in float64 straight from the definition (NOT the engine's bits): good for fixtures of the CPU tests and for a sanity bound on the GPU."""
    U, V, W = np.asarray(U, np.float64), np.asarray(V, np.float64), np.asarray(W, np.float64)
    P = U.shape[1]
    wd = W[0] - W[1]
    delta = (U @ wd[:P])[:, None] + (V @ wd[P:2 * P])[None, :] + np.abs(U[:, None, :] - V[None, :, :]) @ wd[2 * P:]
    p0 = 1.0 / (1.0 + np.exp(-delta))
    return p0 if same_idx == 0 else 1.0 - p0
