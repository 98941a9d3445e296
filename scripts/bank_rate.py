"""The anchor-bank audit, both ways to the same integers (profiles/bank_bench.txt):

  (a) the only route the tree offered before: claims.ClaimIndex.select for all vectors + fetch (every claimed (row, p) pair crosses PCIe), then the definitions of
      tests/bank_kit.py on the host, vectorised (bincounts for totals / hist / sole, one fp32 matrix product per class for the overlap — exact below 2^24 —, and
      the greedy cover over the rows that are still uncovered);
  (b) bank.BankAudit: mark + totals + multiplicity + overlap + greedy to the end; only the integers come back.

Synthetic 512-d embeddings as in scripts/report_index_rate.py, N = 1 048 576 rows, G = 124 and 1 000 vectors, per-vector thresholds at which a vector claims about
3 % of the rows; classes = (claimed by some vector) XOR 15 % noise, so that the greedy cover has rounds to run.  One untimed warm-up of both ways per shape, then
alternating repeats, wall clock between synchronisations (every call returns synchronised), kernel_ms beside the wall time.  Two statements are printed PASS / FAIL:

  1. (b) is faster than (a) at every shape by more than the repeat-to-repeat spread of both, with equal results;
  2. mvb_mark's kernels take no longer than mvc_select's on the same rows and vectors with every threshold at nextafter(1, 2) (nothing is claimed there, so
     mvc_select times exactly its mark + scan phase: the same sweep with the same ending), beyond the spread of both.

  python scripts/bank_rate.py [--rows 1048576] [--vectors 124,1000] [--repeats 3] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from memvul_amd import bank, claims, synth  # noqa: E402
from scripts.report_index_rate import embeddings  # noqa: E402


def audit_a(cx, V, th, cls, n, w_pos, w_neg):
    """-> (dict of the audit's integers, bytes that crossed PCIe towards the host)."""
    G = V.shape[0]
    off, rows, p = cx.select(V, th, order="row")
    down = off.nbytes + rows.nbytes + p.nbytes
    pos = cls.astype(bool)
    q_of = np.repeat(np.arange(G), np.diff(off))
    rpos = pos[rows]
    n1 = np.bincount(q_of[rpos], minlength=G)
    totals = np.stack([np.diff(off) - n1, n1], 1).astype(np.int64)
    m = np.bincount(rows, minlength=n)
    hist = np.stack([np.bincount(m[~pos], minlength=G + 1), np.bincount(m[pos], minlength=G + 1)]).astype(np.int64)
    one = m[rows] == 1
    sole = np.stack([np.bincount(q_of[one & ~rpos], minlength=G), np.bincount(q_of[one & rpos], minlength=G)], 1).astype(np.int64)
    B = np.zeros((n, G), np.uint8)
    B[rows, q_of] = 1
    ov = []
    for sel in (~pos, pos):  # one fp32 product per class and block of rows: every block's counts are below 2^24, so exact; summed in int64
        idx = np.flatnonzero(sel)
        acc = np.zeros((G, G), np.int64)
        for s0 in range(0, len(idx), 131072):
            b = B[idx[s0:s0 + 131072]].astype(np.float32)
            acc += np.rint(b.T @ b).astype(np.int64)
        ov.append(acc)
    overlap = np.stack(ov, 2)
    # greedy: only the rows that are still uncovered are summed
    live = m > 0
    Bp, Bn = B[live & pos], B[live & ~pos]
    taken = np.zeros(G, bool)
    order, gained = [], []
    while len(order) < G:
        npos = np.add.reduce(Bp, axis=0, dtype=np.int64)
        nneg = np.add.reduce(Bn, axis=0, dtype=np.int64)
        gain = np.where(taken, np.iinfo(np.int64).min, w_pos * npos - w_neg * nneg)
        q = int(np.argmax(gain))  # (the first of equal gains: the lowest index)
        if gain[q] <= 0:
            break
        order.append(q)
        gained.append((int(npos[q]), int(nneg[q])))
        taken[q] = True
        Bp, Bn = Bp[Bp[:, q] == 0], Bn[Bn[:, q] == 0]
    return dict(totals=totals, hist=hist, sole=sole, overlap=overlap, order=np.asarray(order, np.int32), gained=np.asarray(gained, np.int64).reshape(-1, 2)), down


def audit_b(bx, V, th, w_pos, w_neg):
    """-> (dict of the audit's integers, bytes that crossed PCIe towards the host, kernel_ms per call)."""
    ms = {}
    bx.mark(V, th)
    ms["mark"] = bx.kernel_ms()
    totals = bx.totals()
    ms["totals"] = bx.kernel_ms()
    hist, sole = bx.multiplicity()
    ms["multiplicity"] = bx.kernel_ms()
    overlap = bx.overlap()
    ms["overlap"] = bx.kernel_ms()
    order, gained = bx.greedy(w_pos, w_neg)
    ms["greedy"] = bx.kernel_ms() if len(order) else 0.0
    out = dict(totals=totals, hist=hist, sole=sole, overlap=overlap, order=order, gained=gained)
    return out, sum(x.nbytes for x in out.values()), ms


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rows", default="1048576")
    ap.add_argument("--vectors", default="124,1000")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--share", type=float, default=0.03)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    dims = synth.BertDims(layers=2, vocab_size=2048)
    Wm = np.ascontiguousarray(synth.make_weights(dims, qk_scale=4.0, match_scale=6.0)[synth.KEY_MATCH_W], np.float32)
    w_pos, w_neg = 1, 1
    say(f"# anchor-bank audit: (a) ClaimIndex.select + fetch + numpy definitions  vs  (b) BankAudit mark + totals + multiplicity + overlap + greedy; {a.repeats} alternating "
        "repeats after a warm-up of both, wall clock in ms")
    ok1 = ok2 = True
    for n in [int(x) for x in a.rows.split(",")]:
        U = embeddings(n, 512, 1)
        with claims.ClaimIndex(0, 512, Wm, 0) as cx, bank.BankAudit(0, 512, Wm, 0) as bx:
            for s0 in range(0, n, 65536):
                cx.add(U[s0:s0 + 65536])
                bx.add(U[s0:s0 + 65536])
            for G in [int(x) for x in a.vectors.split(",")]:
                V = embeddings(G, 512, 2)
                off, _, p = cx.select(V, 0.0, 0, min(n, 8192), order="row")  # (a sample of P(same): the thresholds are quantiles of it)
                th = np.array([np.quantile(p[off[q]:off[q + 1]], 1 - a.share) for q in range(G)], np.float32)
                bx.mark(V, th)
                mult = bx.multiplicity(per_row=True)[2]
                cls = ((mult >= 1) ^ (np.random.default_rng(5).random(n) < 0.15)).astype(np.uint8)
                cx.set_classes(cls)
                bx.set_classes(cls)
                ra, down_a = audit_a(cx, V, th, cls, n, w_pos, w_neg)  # the warm-up of both: first launches load code objects, workspaces grow
                rb, down_b, _ = audit_b(bx, V, th, w_pos, w_neg)
                ta, tb, kms = [], [], []
                same = True
                for _ in range(a.repeats):
                    t0 = time.perf_counter()
                    ra, down_a = audit_a(cx, V, th, cls, n, w_pos, w_neg)
                    ta.append(1e3 * (time.perf_counter() - t0))
                    t0 = time.perf_counter()
                    rb, down_b, ms = audit_b(bx, V, th, w_pos, w_neg)
                    tb.append(1e3 * (time.perf_counter() - t0))
                    kms.append(ms)
                    print(f"  N={n} G={G}: (a) {ta[-1]:.0f} ms, (b) {tb[-1]:.1f} ms", flush=True)  # (progress; the summary line follows)
                    same = same and all(ra[k].dtype == rb[k].dtype and ra[k].shape == rb[k].shape and ra[k].tobytes() == rb[k].tobytes() for k in ra)
                spread = (max(ta) - min(ta)) + (max(tb) - min(tb))
                faster = min(ta) - max(tb) > spread
                ok1 = ok1 and same and faster
                share = float(rb["totals"].sum()) / (n * G)
                say(f"N={n} G={G} (claimed share {100 * share:.2f} %, union TP+FP {int(rb['hist'][:, 1:].sum())}, greedy rounds {len(rb['order'])}): "
                    f"(a) {' '.join(f'{t:.1f}' for t in ta)}  (b) {' '.join(f'{t:.2f}' for t in tb)}  ratio of medians {np.median(ta) / np.median(tb):.0f}x  "
                    f"bytes to the host (a) {down_a} (b) {down_b}  results equal: {same}  (b) faster by more than the spread ({spread:.1f} ms): {faster}")
                for k in ("mark", "totals", "multiplicity", "overlap", "greedy"):
                    say(f"N={n} G={G} kernels of {k}: {' '.join(f'{m[k]:.3f}' for m in kms)} ms")
                # statement 2: the same sweep with the same ending
                none = np.full(G, np.nextafter(np.float32(1), np.float32(2)), np.float32)
                cx.select(V, none, order="row"), bx.mark(V, none)
                kc, kb = [], []
                for _ in range(a.repeats):
                    cx.select(V, none, order="row")
                    kc.append(cx.kernel_ms())
                    bx.mark(V, none)
                    kb.append(bx.kernel_ms())
                spread = (max(kc) - min(kc)) + (max(kb) - min(kb))
                no_longer = np.median(kb) - np.median(kc) <= spread
                ok2 = ok2 and no_longer
                say(f"N={n} G={G} kernels, nothing claimed: mvb_mark {' '.join(f'{t:.2f}' for t in kb)}  mvc_select (mark + scan) {' '.join(f'{t:.2f}' for t in kc)}  "
                    f"mark no longer than select beyond the spread ({spread:.2f} ms): {no_longer}")
    say(f"1. (b) is faster than (a) at every shape by more than the repeat-to-repeat spread of both, with equal results: {'PASS' if ok1 else 'FAIL'}")
    say(f"2. mvb_mark's kernels take no longer than mvc_select's mark + scan on the same rows and vectors, beyond the spread: {'PASS' if ok2 else 'FAIL'}")
    return 0 if ok1 and ok2 else 1


if __name__ == "__main__":
    sys.exit(main())
