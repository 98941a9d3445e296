"""Shared by the anchor-bank audit tests (memvul_amd/bank.py, csrc/bank_cover.h): the definitions of include/memvul_bank.h in numpy, written straight from the
definition (boolean matrices, no words), and a numpy restatement of the kernel plan (64-row ballot words numbered from ``first``, vector groups that write their
slice of the bit matrix, word chunks, the overlap's upper triangle of tiles and its mirror, the greedy pick's reduction and tie rule) that takes seeded faults.
Tests only."""
import numpy as np

import report_index_kit as rkit  # noqa: F401  (the fixture, for the tests that import this kit)

QT = 16         # vectors per tile of the mark kernel (bank_cover.h BK_QT)
OT = 32         # vectors per side of an overlap tile (BK_OT)
PICK = 1024     # threads of the pick kernel (BK_PICK_THREADS)
FAULTS = ("gt", "dead_lanes", "local_class", "tie_high", "fixed_picked", "diag_twice")


# ---- the definitions ---------------------------------------------------------------------------------------------------------------------------------------------------

def marking(p: np.ndarray, thres: np.ndarray) -> np.ndarray:
    """p [N, Q] fp32, thres [Q] fp32 -> bool [N, Q]: vector q claims row n iff p >= thres[q] in IEEE fp32 (a NaN claims nothing)."""
    p, thres = np.asarray(p, np.float32), np.asarray(thres, np.float32)
    with np.errstate(invalid="ignore"):
        return p >= thres[None, :]


def totals(B: np.ndarray, cls: np.ndarray) -> np.ndarray:
    """int64 [Q, 2]: rows of class c that q claims."""
    pos = np.asarray(cls) != 0
    return np.stack([(B & ~pos[:, None]).sum(0), (B & pos[:, None]).sum(0)], 1).astype(np.int64)


def multiplicity(B: np.ndarray, cls: np.ndarray):
    """(hist int64 [2, Q + 1], sole int64 [Q, 2], mult uint16 [N], sole_of int32 [N])."""
    N, Q = B.shape
    cls = (np.asarray(cls) != 0).astype(np.int64)
    m = B.sum(1).astype(np.int64)
    hist = np.zeros((2, Q + 1), np.int64)
    sole = np.zeros((Q, 2), np.int64)
    sole_of = np.full(N, -1, np.int32)
    for n in range(N):
        hist[cls[n], m[n]] += 1
        if m[n] == 1:
            q = int(np.flatnonzero(B[n])[0])
            sole[q, cls[n]] += 1
            sole_of[n] = q
    return hist, sole, m.astype(np.uint16), sole_of


def overlap(B: np.ndarray, cls: np.ndarray) -> np.ndarray:
    """int64 [Q, Q, 2]: rows of class c that q and r both claim."""
    pos = np.asarray(cls) != 0
    b1, b0 = (B & pos[:, None]).astype(np.int64), (B & ~pos[:, None]).astype(np.int64)
    return np.stack([b0.T @ b0, b1.T @ b1], 2)


def greedy(B: np.ndarray, cls: np.ndarray, w_pos: int, w_neg: int, fixed=None, max_rounds=None):
    """(order int32 [rounds], gained int64 [rounds, 2], tied): the greedy cover of include/memvul_bank.h in Python integers; ``tied`` counts the rounds whose
    winning gain was shared by at least two candidates."""
    N, Q = B.shape
    pos = np.asarray(cls) != 0
    fixed = np.zeros(Q, bool) if fixed is None else np.asarray(fixed) != 0
    max_rounds = Q if max_rounds is None else max_rounds
    covered = B[:, fixed].any(1) if fixed.any() else np.zeros(N, bool)
    taken = fixed.copy()
    order, gained, tied = [], [], 0
    while len(order) < max_rounds:
        best = None
        gains = {}
        for q in range(Q):
            if taken[q]:
                continue
            new = B[:, q] & ~covered
            npos, nneg = int((new & pos).sum()), int((new & ~pos).sum())
            gains[q] = (int(w_pos) * npos - int(w_neg) * nneg, npos, nneg)
            if best is None or gains[q][0] > gains[best][0]:  # (ascending q: the lowest index keeps a tie)
                best = q
        if best is None or gains[best][0] <= 0:
            break
        tied += sum(1 for g in gains.values() if g[0] == gains[best][0]) > 1
        order.append(best)
        gained.append(gains[best][1:])
        taken[best] = True
        covered = covered | B[:, best]
    return np.asarray(order, np.int32), np.asarray(gained, np.int64).reshape(-1, 2), tied


def mark_bytes(Q: int, count: int) -> int:
    """The bytes of a held marking, restated: 8 per vector and started word of 64 rows."""
    return 8 * Q * -(-count // 64)


# ---- the plan -------------------------------------------------------------------------------------------------------------------------------------------------------------

def _popcount(x) -> np.ndarray:
    x = np.ascontiguousarray(np.asarray(x, np.uint64))
    return np.unpackbits(x.view(np.uint8).reshape(x.shape + (8,)), axis=-1).sum((-1, -2)).astype(np.int64)


def _pack(bits: np.ndarray) -> np.ndarray:
    """bool [..., 64 k] -> uint64 [..., k], bit l of word w = entry 64 w + l."""
    b = np.asarray(bits, bool)
    b = b.reshape(b.shape[:-1] + (-1, 64)).astype(np.uint64)
    return (b << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)


def plan_mark(p, cls, thres, first, count, block_rows, vector_group, fault=None):
    """The mark pass: (bits uint64 [Q, W], posword uint64 [W]).  Vectors in groups of vector_group, each writing its slice of the full matrix; tiles of QT; blocks
    of block_rows rows numbered from ``first``; per wave one ballot word per vector.  Dead lanes hold a NaN — or, under "dead_lanes", the block's last live value;
    "gt": > for >=; "local_class": the class words read the classes at the range-local row."""
    p, cls, thres = np.asarray(p, np.float32), np.asarray(cls), np.asarray(thres, np.float32)
    Q = p.shape[1]
    W = (count + 63) // 64
    bits = np.zeros((Q, W), np.uint64)
    nw = block_rows // 64
    nblocks = (count + block_rows - 1) // block_rows
    for q0 in range(0, Q, vector_group):
        nq = min(vector_group, Q - q0)
        slice_ = np.zeros((nq, W), np.uint64)  # the group's slice
        for t0 in range(0, nq, QT):
            for b in range(nblocks):
                r0 = b * block_rows
                live = min(block_rows, count - r0)
                for j in range(min(QT, nq - t0)):
                    col = p[first + r0:first + r0 + live, q0 + t0 + j]
                    pad = np.full(block_rows - live, col[-1] if fault == "dead_lanes" else np.float32("nan"), np.float32)
                    x = np.concatenate([col, pad])
                    with np.errstate(invalid="ignore"):
                        hit = (x > thres[q0 + t0 + j]) if fault == "gt" else (x >= thres[q0 + t0 + j])
                    words = _pack(hit)
                    for w in range(nw):
                        if b * nw + w < W:
                            slice_[t0 + j, b * nw + w] = words[w]
        bits[q0:q0 + nq] = slice_
    r = np.arange(W * 64)
    at = np.minimum(r, max(count - 1, 0)) + (0 if fault == "local_class" else first)
    pos = _pack((r < count) & (cls[at] != 0)) if count else np.zeros(0, np.uint64)
    return bits, pos


def plan_totals(bits, pos):
    """One workgroup per vector: its words met with the class words."""
    return np.stack([np.array([int(_popcount(row & ~pos)) for row in bits], np.int64), np.array([int(_popcount(row & pos)) for row in bits], np.int64)], 1).reshape(-1, 2)


def plan_multiplicity(bits, pos, count, word_chunk):
    """A workgroup owns word_chunk consecutive words; lane = row; per-workgroup histogram and sole counts, then added into the results."""
    Q, W = bits.shape
    hist, sole = np.zeros((2, Q + 1), np.int64), np.zeros((Q, 2), np.int64)
    mult, sole_of = np.zeros(count, np.uint16), np.full(count, -1, np.int32)
    lanes = np.arange(64, dtype=np.uint64)
    for w0 in range(0, W, word_chunk):
        lh, ls = np.zeros((2, Q + 1), np.int64), np.zeros((Q, 2), np.int64)
        for w in range(w0, min(w0 + word_chunk, W)):
            bit = ((bits[:, w][:, None] >> lanes[None, :]) & np.uint64(1)).astype(np.int64)  # [Q, 64]
            m = bit.sum(0)
            who = np.where(bit.any(0), Q - 1 - np.argmax(bit[::-1], 0), -1)  # the last claimant
            c = ((pos[w] >> lanes) & np.uint64(1)).astype(np.int64)
            for l in range(64):
                r = 64 * w + l
                if r < count:
                    lh[c[l], m[l]] += 1
                    if m[l] == 1:
                        ls[who[l], c[l]] += 1
                    mult[r] = m[l]
                    sole_of[r] = who[l] if m[l] == 1 else -1
        hist += lh
        sole += ls
    return hist, sole, mult, sole_of


def plan_overlap(bits, pos, word_chunk, fault=None):
    """Tiles of OT x OT vectors, the upper triangle of tiles only and, in a diagonal tile, only q <= r; word chunks added into the result; then the mirror copies
    the upper triangle below the diagonal.  "diag_twice": the mirror ADDS the transposed tile instead, diagonal tiles included."""
    Q, W = bits.shape
    out = np.zeros((Q, Q, 2), np.int64)
    nt = (Q + OT - 1) // OT
    for a in range(nt):
        for b in range(a, nt):
            for w0 in range(0, W, word_chunk):
                ws = slice(w0, min(w0 + word_chunk, W))
                for q in range(a * OT, min(a * OT + OT, Q)):
                    for r in range(b * OT, min(b * OT + OT, Q)):
                        if a == b and q > r:
                            continue
                        x = bits[q, ws] & bits[r, ws]
                        n, n1 = int(_popcount(x)), int(_popcount(x & pos[ws]))
                        out[q, r, 0] += n - n1
                        out[q, r, 1] += n1
    if fault == "diag_twice":
        for a in range(nt):
            for b in range(a, nt):
                qa, qb = slice(a * OT, min(a * OT + OT, Q)), slice(b * OT, min(b * OT + OT, Q))
                out[qb, qa] = out[qb, qa] + out[qa, qb].transpose(1, 0, 2)
        return out
    for q in range(Q):
        for r in range(q):
            out[q, r] = out[r, q]
    return out


def plan_greedy(bits, pos, word_chunk, w_pos, w_neg, fixed=None, max_rounds=None, fault=None, look_every=8):
    """Per round: partial gains per (vector, word chunk) over ~covered; the pick: thread t takes vectors t, t + PICK, .. (a later equal gain does not replace an
    earlier one), then a tree over the threads by (gain descending, index ascending); the pick's row is ORed into ``covered``.  A sticky ``done`` turns later rounds
    into no-ops; the host looks every ``look_every`` rounds.  "tie_high": ties to the higher index; "fixed_picked": the fixed mask is lost (its vectors cover nothing and
    can be picked)."""
    Q, W = bits.shape
    fixed = np.zeros(Q, bool) if fixed is None else np.asarray(fixed) != 0
    limit = min(Q if max_rounds is None else max_rounds, int((~fixed).sum()))
    order, gained = [], []
    if W == 0 or limit == 0 or w_pos == 0:
        return np.zeros(0, np.int32), np.zeros((0, 2), np.int64)
    covered = np.zeros(W, np.uint64)
    taken = fixed.copy()
    if fault == "fixed_picked":  # (the mask never reaches the device: a fixed vector covers nothing and can be picked)
        taken[:] = False
    for q in np.flatnonzero(taken):
        covered |= bits[q]
    done, r = False, 0
    nchunks = (W + word_chunk - 1) // word_chunk

    def better(a, b):  # does candidate b = (gain, q, ..) beat a?
        if b is None:
            return False
        if a is None or b[0] > a[0]:
            return True
        return b[0] == a[0] and (b[1] > a[1] if fault == "tie_high" else b[1] < a[1])

    while r < limit and not done:  # the host's loop: `look_every` rounds are enqueued, then it looks at `done`
        upto = min(limit, r + look_every)
        while r < upto:
            r += 1
            if done:  # (a launch after `done` does nothing)
                continue
            part = np.zeros((Q, nchunks, 2), np.int64)
            for q in range(Q):
                if taken[q]:
                    continue
                for c in range(nchunks):
                    ws = slice(c * word_chunk, min((c + 1) * word_chunk, W))
                    x = bits[q, ws] & ~covered[ws]
                    n1 = int(_popcount(x & pos[ws]))
                    part[q, c] = (int(_popcount(x)) - n1, n1)
            threads = [None] * PICK
            for q in range(Q):
                if taken[q]:
                    continue
                n0, n1 = int(part[q, :, 0].sum()), int(part[q, :, 1].sum())
                cand = (int(w_pos) * n1 - int(w_neg) * n0, q, n1, n0)
                t = q % PICK
                if threads[t] is None or (cand[0] >= threads[t][0] if fault == "tie_high" else cand[0] > threads[t][0]):
                    threads[t] = cand
            step = PICK // 2
            while step:
                for t in range(step):
                    if better(threads[t], threads[t + step]):
                        threads[t] = threads[t + step]
                step //= 2
            best = threads[0]
            if best is None or best[0] <= 0:
                done = True
                continue
            order.append(best[1])
            gained.append((best[2], best[3]))
            taken[best[1]] = True
            covered = covered | bits[best[1]]
    return np.asarray(order, np.int32), np.asarray(gained, np.int64).reshape(-1, 2)


def plan_audit(p, cls, thres, first, count, block_rows, vector_group, word_chunk, w_pos=1, w_neg=1, fixed=None, max_rounds=None, fault=None, look_every=8):
    """Every result of the library for one marking, through the plan: a dict with bits, totals, hist, sole, mult, sole_of, overlap, order, gained."""
    bits, pos = plan_mark(p, cls, thres, first, count, block_rows, vector_group, fault)
    hist, sole, mult, sole_of = plan_multiplicity(bits, pos, count, word_chunk)
    order, gained = plan_greedy(bits, pos, word_chunk, w_pos, w_neg, fixed, max_rounds, fault, look_every)
    return dict(bits=bits, totals=plan_totals(bits, pos), hist=hist, sole=sole, mult=mult, sole_of=sole_of, overlap=plan_overlap(bits, pos, word_chunk, fault),
                order=order, gained=gained)


def definition_audit(p, cls, thres, first, count, w_pos=1, w_neg=1, fixed=None, max_rounds=None):
    """The same dict straight from the definitions, over rows [first, first + count)."""
    B = marking(np.asarray(p)[first:first + count], thres)
    c = np.asarray(cls)[first:first + count]
    hist, sole, mult, sole_of = multiplicity(B, c)
    order, gained, tied = greedy(B, c, w_pos, w_neg, fixed, max_rounds)
    W = (count + 63) // 64
    padded = np.zeros((W * 64, B.shape[1]), bool)
    padded[:count] = B
    return dict(bits=_pack(padded.T) if W else np.zeros((B.shape[1], 0), np.uint64), totals=totals(B, c), hist=hist, sole=sole, mult=mult, sole_of=sole_of,
                overlap=overlap(B, c), order=order, gained=gained, tied=tied)


def same(a: dict, b: dict, keys=("bits", "totals", "hist", "sole", "mult", "sole_of", "overlap", "order", "gained")) -> list:
    """The keys on which two result dicts differ (dtype, shape or a byte)."""
    return [k for k in keys if np.asarray(a[k]).dtype != np.asarray(b[k]).dtype or np.asarray(a[k]).shape != np.asarray(b[k]).shape
            or np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes()]


def bits_of_selection(offsets, rows, Q: int, first: int, count: int) -> np.ndarray:
    """The bit matrix that a row-ordered selection (ClaimIndex.select(order="row")) stands for: uint64 [Q, ceil(count / 64)], words numbered from ``first``."""
    W = (count + 63) // 64
    B = np.zeros((Q, W * 64), bool)
    for q in range(Q):
        B[q, np.asarray(rows[offsets[q]:offsets[q + 1]], np.int64) - first] = True
    return _pack(B) if W else np.zeros((Q, 0), np.uint64)
