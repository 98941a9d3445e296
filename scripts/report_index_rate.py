"""Per-anchor retrieval, both ways to the same answer (profiles/report_index_bench.txt):

  (a) what the engine alone offers: Engine.match in batches of max_batch with P(same) downloaded, then per column numpy.partition for the k-th key, and a sort of the
      rows at or above it by (key descending, row ascending);
  (b) retrieve.ReportIndex.query over an index filled once (the fill — add from host memory — is timed by itself).

Synthetic embeddings, N = 65 536 and 1 048 576 rows, G = 124 and 1 000 query vectors, k = 10, three alternating repeats after one untimed warm-up of both ways per shape; wall clock between synchronisations (both
calls return synchronised), plus mvr_kernel_ms for (b).  The bytes of the two answers are compared.  The statement printed at the end: (b) is faster than (a) at every
shape by more than the repeat-to-repeat spread of the two.

  python scripts/report_index_rate.py [--rows 65536,1048576] [--vectors 124,1000] [--k 10] [--repeats 3] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from memvul_amd import retrieve, synth  # noqa: E402
from memvul_amd.binding import Engine  # noqa: E402


def embeddings(n, P, seed):
    """Non-negative, about half zeros (the header's output is a ReLU)."""
    rng = np.random.default_rng(seed)
    out = np.empty((n, P), np.float32)
    for s0 in range(0, n, 65536):
        m = min(65536, n - s0)
        out[s0:s0 + m] = np.maximum(rng.standard_normal((m, P), dtype=np.float32), 0) * rng.uniform(0.2, 1.5, (m, 1)).astype(np.float32)
    return out


def host_topk(ps, k):
    """(a)'s ranking: ps [N, G] -> (p [G, k], rows [G, k]) in the order (key descending, row ascending), key(NaN) = 2."""
    N, G = ps.shape
    pt = np.ascontiguousarray(ps.T)
    top_p, rows = np.full((G, k), -1.0, np.float32), np.full((G, k), -1, np.int64)
    kk = min(k, N)
    for g in range(G):
        col = pt[g]
        key = np.where(np.isnan(col), np.float32(2.0), col)
        kth = np.partition(key, N - kk)[N - kk]
        cand = np.flatnonzero(key >= kth)
        order = cand[np.lexsort((cand, -key[cand].astype(np.float64)))][:kk]
        top_p[g, :kk], rows[g, :kk] = col[order], order
    return top_p, rows


def way_a(eng, U, V, k):
    eng.anchor_set(V)
    mb = eng.cfg.max_batch
    ps = np.empty((U.shape[0], V.shape[0]), np.float32)
    for s0 in range(0, U.shape[0], mb):
        ps[s0:s0 + mb] = eng.match(U[s0:s0 + mb])["probs"][:, :, 0]
    t1 = time.perf_counter()
    out = host_topk(ps, k)
    return out, time.perf_counter() - t1


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rows", default="65536,1048576")
    ap.add_argument("--vectors", default="124,1000")
    ap.add_argument("--k", type=int, default=10)
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
    w = synth.make_weights(dims, qk_scale=4.0, match_scale=6.0)
    Wm = np.ascontiguousarray(w[synth.KEY_MATCH_W], np.float32)
    eng = Engine(0, vocab_size=dims.vocab_size, layers=dims.layers, max_tokens=16384, max_batch=512, max_anchors=1024)
    eng.load_state_dict(w)
    say(f"# per-anchor retrieval: (a) Engine.match + download + numpy ranking  vs  (b) ReportIndex.query; k = {a.k}, {a.repeats} alternating repeats after a warm-up, wall clock in ms")
    ok = True
    for n in [int(x) for x in a.rows.split(",")]:
        U = embeddings(n, 512, 1)
        with retrieve.ReportIndex(0, 512, Wm, 0) as ix:
            t0 = time.perf_counter()
            for s0 in range(0, n, 65536):
                ix.add(U[s0:s0 + 65536])
            say(f"N={n}: fill (add from host memory, 65536 rows per call) {1e3 * (time.perf_counter() - t0):.1f} ms")
            for G in [int(x) for x in a.vectors.split(",")]:
                V = embeddings(G, 512, 2)
                ta, tb, tk, trank = [], [], [], []
                same = True
                way_a(eng, U[:4 * eng.cfg.max_batch], V, a.k)  # warm-up of every shape the timed window uses: first launches load code objects, workspaces grow
                ix.query(V, a.k)
                for _ in range(a.repeats):
                    t0 = time.perf_counter()
                    (pa, ra), rank_s = way_a(eng, U, V, a.k)
                    ta.append(1e3 * (time.perf_counter() - t0))
                    trank.append(1e3 * rank_s)
                    t0 = time.perf_counter()
                    pb, rb = ix.query(V, a.k)
                    tb.append(1e3 * (time.perf_counter() - t0))
                    tk.append(ix.kernel_ms())
                    same = same and pa.tobytes() == pb.tobytes() and np.array_equal(ra, rb)
                spread = (max(ta) - min(ta)) + (max(tb) - min(tb))
                faster = min(ta) - max(tb) > spread
                ok = ok and same and faster
                say(f"N={n} G={G}: (a) {' '.join(f'{t:.1f}' for t in ta)} (of which host ranking {' '.join(f'{t:.1f}' for t in trank)})  "
                    f"(b) {' '.join(f'{t:.2f}' for t in tb)} (kernels {' '.join(f'{t:.2f}' for t in tk)})  "
                    f"ratio of medians {np.median(ta) / np.median(tb):.0f}x  bytes equal: {same}  (b) faster by more than the spread ({spread:.1f} ms): {faster}")
    eng.close()
    say(f"(b) is faster than (a) at every shape by more than the repeat-to-repeat spread of the two, with equal bytes: {ok}")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
