"""Per-anchor claims, both ways to the same answer (profiles/claims_bench.txt):

  (a) what the tree offered before: retrieve.ReportIndex.psame in calls of at most 2^28 values, P(same) downloaded, then on the host `>=` and nonzero per column
      (select), or the number of thresholds each value reaches and one bincount split by class (counts);
  (b) claims.ClaimIndex.select at one threshold that claims about 0.32 % of the pairs (the corpus' positive rate) and one that claims about 10 %, and
      claims.ClaimIndex.counts at the reference's 40 thresholds.

Synthetic 512-d embeddings as in scripts/report_index_rate.py, N = 65 536 and 1 048 576 rows, G = 124 and 1 000 vectors; one untimed warm-up of both ways per shape,
three alternating repeats, wall clock between synchronisations (every call returns synchronised), the bytes of both answers compared, kernel_ms beside the wall time.
Two statements are printed PASS / FAIL:

  1. (b) is faster than (a) at every shape by more than the repeat-to-repeat spread of both;
  2. the kernels of counts at T = 40 take no longer than those of ReportIndex.query at k = 10 on the same rows and vectors, beyond the spread of both.

  python scripts/claims_rate.py [--rows 65536,1048576] [--vectors 124,1000] [--repeats 3] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from memvul_amd import claims, retrieve, synth  # noqa: E402
from scripts.report_index_rate import embeddings  # noqa: E402


def psame_chunks(rx, V, n):
    """(a)'s matrix, in calls of at most 2^28 values: yields (first row, P(same) [rows, G])."""
    step = max(1, retrieve.MAX_PSAME // V.shape[0])
    for s0 in range(0, n, step):
        yield s0, rx.psame(V, s0, min(step, n - s0))


def select_a(rx, V, n, t32):
    """-> (offsets, rows, p) in row order; t32: fp32 [G]."""
    G = V.shape[0]
    rows, ps = [[] for _ in range(G)], [[] for _ in range(G)]
    for s0, p in psame_chunks(rx, V, n):
        hit = p >= t32[None, :]
        r, g = np.nonzero(hit.T)[::-1]  # (vector-major: each vector's rows ascending)
        cut = np.searchsorted(g, np.arange(G + 1))
        val = p[r, g]
        for q in range(G):
            rows[q].append(r[cut[q]:cut[q + 1]] + s0)
            ps[q].append(val[cut[q]:cut[q + 1]])
    rows = [np.concatenate(x) for x in rows]
    off = np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.int64)
    return off, np.concatenate(rows).astype(np.int64), np.concatenate([np.concatenate(x) for x in ps]).astype(np.float32)


def counts_a(rx, V, n, cls, t32):
    """-> int64 [G, T, 2]: per value the number of thresholds it reaches (a NaN reaches none), one bincount split by vector and class, a suffix sum."""
    G, T = V.shape[0], len(t32)
    order = np.argsort(t32, kind="stable")
    srt = t32[order]
    hist = np.zeros((G, 2, T + 1), np.int64)
    for s0, p in psame_chunks(rx, V, n):
        m = np.searchsorted(srt, p, side="right")
        m[np.isnan(p)] = 0
        key = m + (T + 1) * (cls[s0:s0 + len(p), None].astype(np.int64) + 2 * np.arange(G)[None, :])
        hist += np.bincount(key.reshape(-1), minlength=G * 2 * (T + 1)).reshape(G, 2, T + 1)
    reach = hist[:, :, ::-1].cumsum(2)[:, :, ::-1]  # [g, c, m]: values that reach at least m of the sorted thresholds
    out = np.empty((G, T, 2), np.int64)
    out[:, order, :] = reach[:, :, 1:].transpose(0, 2, 1)
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rows", default="65536,1048576")
    ap.add_argument("--vectors", default="124,1000")
    ap.add_argument("--repeats", type=int, default=3)
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
    grid = claims.reference_grid()
    say(f"# per-anchor claims: (a) ReportIndex.psame + download + numpy  vs  (b) ClaimIndex.select / counts; {a.repeats} alternating repeats after a warm-up of both, wall clock in ms")
    ok1 = ok2 = True
    for n in [int(x) for x in a.rows.split(",")]:
        U = embeddings(n, 512, 1)
        cls = (np.random.default_rng(3).random(n) < 0.0032).astype(np.uint8)
        with retrieve.ReportIndex(0, 512, Wm, 0) as rx, claims.ClaimIndex(0, 512, Wm, 0) as cx:
            t0 = time.perf_counter()
            for s0 in range(0, n, 65536):
                cx.add(U[s0:s0 + 65536])
            cx.set_classes(cls)
            say(f"N={n}: fill of the claim index (add from host memory, 65536 rows per call, and the classes) {1e3 * (time.perf_counter() - t0):.1f} ms")
            for s0 in range(0, n, 65536):
                rx.add(U[s0:s0 + 65536])
            for G in [int(x) for x in a.vectors.split(",")]:
                V = embeddings(G, 512, 2)
                sample = rx.psame(V, 0, min(n, 8192))
                jobs = [(f"select ~{100 * s:.2f} %", np.full(G, np.quantile(sample, 1 - s), np.float32)) for s in (0.0032, 0.10)] + [("counts T=40", grid)]
                for what, th in jobs:
                    is_counts = what.startswith("counts")
                    way_a = (lambda: counts_a(rx, V, n, cls, th)) if is_counts else (lambda: select_a(rx, V, n, th))
                    way_b = (lambda: cx.counts(V, th)) if is_counts else (lambda: cx.select(V, th, order="row"))
                    way_a(), way_b()  # the warm-up: first launches load code objects, workspaces grow
                    ta, tb, tk = [], [], []
                    same = True
                    for _ in range(a.repeats):
                        t0 = time.perf_counter()
                        ra = way_a()
                        ta.append(1e3 * (time.perf_counter() - t0))
                        t0 = time.perf_counter()
                        rb = way_b()
                        tb.append(1e3 * (time.perf_counter() - t0))
                        tk.append(cx.kernel_ms())
                        pairs_a = (ra,) if is_counts else ra
                        pairs_b = (rb,) if is_counts else rb
                        same = same and all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(pairs_a, pairs_b))
                    spread = (max(ta) - min(ta)) + (max(tb) - min(tb))
                    faster = min(ta) - max(tb) > spread
                    ok1 = ok1 and same and faster
                    share = (float(rb[:, :, :].sum(2)[:, 0].sum()) / (n * G)) if is_counts else float(rb[0][-1]) / (n * G)
                    say(f"N={n} G={G} {what} (claimed share {100 * share:.2f} %{' at the first threshold' if is_counts else ''}): (a) {' '.join(f'{t:.1f}' for t in ta)}  "
                        f"(b) {' '.join(f'{t:.2f}' for t in tb)} (kernels {' '.join(f'{t:.2f}' for t in tk)})  ratio of medians {np.median(ta) / np.median(tb):.0f}x  "
                        f"bytes equal: {same}  (b) faster by more than the spread ({spread:.1f} ms): {faster}")
                # statement 2: the same sweep with a cheaper ending?
                rx.query(V, 10), cx.counts(V, grid)
                kq, kc = [], []
                for _ in range(a.repeats):
                    rx.query(V, 10)
                    kq.append(rx.kernel_ms())
                    cx.counts(V, grid)
                    kc.append(cx.kernel_ms())
                spread = (max(kq) - min(kq)) + (max(kc) - min(kc))
                no_longer = np.median(kc) - np.median(kq) <= spread
                ok2 = ok2 and no_longer
                say(f"N={n} G={G} kernels: counts T=40 {' '.join(f'{t:.2f}' for t in kc)}  query k=10 {' '.join(f'{t:.2f}' for t in kq)}  "
                    f"counts no longer than query beyond the spread ({spread:.2f} ms): {no_longer}")
    say(f"1. (b) is faster than (a) at every shape by more than the repeat-to-repeat spread of both, with equal bytes: {'PASS' if ok1 else 'FAIL'}")
    say(f"2. the kernels of counts at T = 40 take no longer than those of query at k = 10 on the same rows and vectors, beyond the spread: {'PASS' if ok2 else 'FAIL'}")
    return 0 if ok1 and ok2 else 1


if __name__ == "__main__":
    sys.exit(main())
