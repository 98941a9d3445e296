"""Shared by the per-anchor claims tests (memvul_amd/claims.py, csrc/claim_sweep.h): the rule in numpy straight from its definition, a numpy restatement of the
kernel plan (tiles -> 64-row ballot words -> per-block partial counts -> fold; word population counts -> scan -> fill) that takes seeded faults, and the thresholds
the GPU tests take from the reference matrix.  Tests only."""
import numpy as np

import report_index_kit as rkit  # noqa: F401  (the fixture and the retrieval order, for the tests that import this kit)

QT = 16  # vectors per tile (claim_sweep.h CL_QT)


def reference_counts(p: np.ndarray, cls: np.ndarray, thresholds: np.ndarray) -> np.ndarray:
    """p [N, Q] fp32, cls [N] in {0, 1}, thresholds [T] fp32 -> int64 [Q, T, 2]: rows of class c with p >= t, in IEEE fp32 (a NaN claims nothing)."""
    p, cls, th = np.asarray(p, np.float32), np.asarray(cls), np.asarray(thresholds, np.float32)
    out = np.zeros((p.shape[1], len(th), 2), np.int64)
    with np.errstate(invalid="ignore"):
        for t, x in enumerate(th):
            claimed = p >= x
            out[:, t, 1] = (claimed & (cls[:, None] != 0)).sum(0)
            out[:, t, 0] = claimed.sum(0) - out[:, t, 1]
    return out


def reference_select(p: np.ndarray, thres: np.ndarray, first: int = 0):
    """p [N, Q], thres [Q] -> (offsets int64 [Q + 1], rows int64, p fp32) in row order: per vector the rows with p >= its threshold, ascending, numbered from
    ``first``; the p handed back are the input's own bits."""
    p, thres = np.asarray(p, np.float32), np.asarray(thres, np.float32)
    rows, ps, offsets = [], [], [0]
    with np.errstate(invalid="ignore"):
        for g in range(p.shape[1]):
            r = np.flatnonzero(p[:, g] >= thres[g])
            rows.append(r + first)
            ps.append(p[r, g])
            offsets.append(offsets[-1] + len(r))
    return (np.asarray(offsets, np.int64), np.concatenate(rows).astype(np.int64) if rows else np.zeros(0, np.int64),
            np.concatenate(ps).astype(np.float32) if ps else np.zeros(0, np.float32))


def by_prob(offsets, rows, p):
    """Each segment re-ordered (P descending, row ascending), written apart from the code under test."""
    rows, p = np.array(rows), np.array(p)
    for g in range(len(offsets) - 1):
        a, b = int(offsets[g]), int(offsets[g + 1])
        order = sorted(range(a, b), key=lambda i: (-float(p[i]), int(rows[i])))
        rows[a:b], p[a:b] = rows[order], p[order]
    return rows, p


def _words(p_block: np.ndarray, th: float, fault: str = None):
    """The ballot words of one block's rows for one vector: list of python ints, bit l of word w = row 64 w + l claimed.  p_block is padded to whole words with
    NaN (a dead lane), or, under the fault "dead_lanes", with the block's last live value."""
    n = len(p_block)
    nw = (n + 63) // 64
    pad = np.full(nw * 64 - n, p_block[-1] if fault == "dead_lanes" else np.float32("nan"), np.float32)
    x = np.concatenate([p_block, pad])
    with np.errstate(invalid="ignore"):
        bits = (x > th) if fault == "gt" else (x >= th)
    return [int(sum(1 << l for l in np.flatnonzero(bits[64 * w:64 * w + 64]).tolist())) for w in range(nw)]


def plan_counts(p: np.ndarray, cls: np.ndarray, thresholds, first: int, count: int, block_rows: int, vector_group: int, fault: str = None) -> np.ndarray:
    """The counts plan of claim_sweep.h over rows [first, first + count) of p [N, Q]: vectors in groups, tiles of QT, blocks of block_rows rows numbered from
    ``first``, per wave one ballot word per (vector, threshold) met with the wave's class word, the block's packed partial (class 0 | class 1 << 16), then the
    fold.  fault: "gt" (> for >=), "dead_lanes" (the last partial word's dead lanes counted), "local_class" (classes read at the block-local row)."""
    p, cls = np.asarray(p, np.float32), np.asarray(cls)
    Q, T = p.shape[1], len(thresholds)
    out = np.zeros((Q, T, 2), np.int64)
    if count == 0:
        return out
    nblocks = (count + block_rows - 1) // block_rows
    for q0 in range(0, Q, vector_group):
        nq = min(vector_group, Q - q0)
        part = np.zeros((nq, nblocks, T), np.uint32)
        for t0 in range(0, nq, QT):
            for b in range(nblocks):
                r0 = b * block_rows
                live = min(block_rows, count - r0)
                at = np.arange(live) if fault == "local_class" else first + r0 + np.arange(live)
                c = np.concatenate([cls[at] != 0, np.zeros((-live) % 64, bool)])
                cw = [int(sum(1 << l for l in np.flatnonzero(c[64 * w:64 * w + 64]).tolist())) for w in range(len(c) // 64)]
                for j in range(min(QT, nq - t0)):
                    col = p[first + r0:first + r0 + live, q0 + t0 + j]
                    for t, th in enumerate(thresholds):
                        s = 0
                        for w, word in enumerate(_words(col, th, fault)):
                            n, n1 = bin(word).count("1"), bin(word & cw[w]).count("1")
                            s += (n - n1) | (n1 << 16)
                        part[t0 + j, b, t] = s
        out[q0:q0 + nq, :, 0] = (part & 0xFFFF).astype(np.int64).sum(1)
        out[q0:q0 + nq, :, 1] = (part >> 16).astype(np.int64).sum(1)
    return out


def plan_select(p: np.ndarray, thres, first: int, count: int, block_rows: int, vector_group: int, fault: str = None):
    """The select plan: mark (the bit matrix [vector][ceil(count / 64)], words numbered from ``first``), scan (word bases, totals, offsets), fill (row and p at
    offsets[q] + base[word] + set bits below the lane).  Returns what reference_select returns.  fault: "gt", "dead_lanes", "word_base" (a word's base is that
    of the word before), "no_first" (``first`` dropped from the row numbers)."""
    p = np.asarray(p, np.float32)
    Q = p.shape[1]
    W = (count + 63) // 64
    nblocks = (count + block_rows - 1) // block_rows if count else 0
    nw = block_rows // 64
    totals, held = np.zeros(Q, np.int64), {}
    for q0 in range(0, Q, vector_group):
        nq = min(vector_group, Q - q0)
        bits = [[0] * W for _ in range(nq)]
        for b in range(nblocks):
            r0 = b * block_rows
            live = min(block_rows, count - r0)
            for j in range(nq):
                for w, word in enumerate(_words(p[first + r0:first + r0 + live, q0 + j], thres[q0 + j], fault)):
                    if b * nw + w < W:
                        bits[j][b * nw + w] = word
        for j in range(nq):
            base, below = [], 0
            for w in range(W):
                base.append(below)
                below += bin(bits[j][w]).count("1")
            if fault == "word_base":
                base = [0] + base[:-1]
            totals[q0 + j] = below
            held[q0 + j] = (bits[j], base)
    offsets = np.concatenate([[0], np.cumsum(totals)]).astype(np.int64)
    rows, ps = np.full(int(offsets[-1]), -1, np.int64), np.full(int(offsets[-1]), -1.0, np.float32)
    for q in range(Q):
        bits, base = held[q]
        for w in range(W):
            word, k = bits[w], 0
            for l in range(64):
                if (word >> l) & 1:
                    o = int(offsets[q]) + base[w] + k
                    k += 1
                    r = 64 * w + l
                    if r < count and o < len(rows):
                        rows[o] = r if fault == "no_first" else first + r
                        ps[o] = p[first + r, q]
    return offsets, rows, ps


def matrix_thresholds(ps: np.ndarray) -> np.ndarray:
    """Thresholds taken FROM a reference matrix ps [N, Q] (fp32): per vector its 0 / 50 / 99.7 / 100th percentile VALUES (order statistics of the non-NaN column, so
    each equals an entry exactly), each one's nextafter up and down, and 0.0, 1.0 and 1.0's nextafter up -> fp32 [Q, 15]."""
    ps = np.asarray(ps, np.float32)
    out = np.zeros((ps.shape[1], 15), np.float32)
    for g in range(ps.shape[1]):
        col = np.sort(ps[:, g][~np.isnan(ps[:, g])])
        if len(col) == 0:
            col = np.array([0.5], np.float32)
        picks = np.array([col[min(len(col) - 1, int(round(f * (len(col) - 1))))] for f in (0.0, 0.5, 0.997, 1.0)], np.float32)
        out[g] = np.concatenate([picks, np.nextafter(picks, np.float32(2)), np.nextafter(picks, np.float32(-1)),
                                 np.array([0.0, 1.0, np.nextafter(np.float32(1), np.float32(2))], np.float32)])
    return out
