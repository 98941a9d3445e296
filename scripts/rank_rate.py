"""Per-anchor ranking quality, both ways to the same numbers (profiles/rank_bench.txt):

  (a) the route a user had before: the P(same) matrix on the host (retrieve.ReportIndex.psame in calls of at most 2^28 values, downloaded), then per anchor
      sklearn's roc_curve + auc and average_precision_score, and the best F1 over precision_recall_curve.  Timed on 8 anchors and SCALED to the number of vectors
      (the matrix itself is timed in full): the line says so;
  (b) rank.RankIndex.rank: score, sort and statistics on the device, a few numbers per anchor back.

Synthetic 512-d embeddings as in scripts/report_index_rate.py, 1.2 M rows, 124 and 1 000 vectors, classes positive at 0.32 %; one untimed warm-up, then repeats, wall
clock between synchronisations (every call returns synchronised).  kernel_ms is split into the score / sort / statistics stages, the rate is rows x vectors per second
of kernel time, and the file states which stage bounds the call.  AUC and AP of the 8 anchors are compared between the two ways (to 1e-12).

  python scripts/rank_rate.py [--rows 1200000] [--vectors 124,1000] [--repeats 3] [--host-anchors 8] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from memvul_amd import rank, retrieve, synth  # noqa: E402
from scripts.report_index_rate import embeddings  # noqa: E402


def host_route(rx, V, n, cls, anchors):
    """-> (seconds for the whole matrix on the host, seconds of sklearn for ``anchors`` columns, their (auc, ap, best f1))."""
    from sklearn import metrics

    G = V.shape[0]
    step = max(1, retrieve.MAX_PSAME // G)
    t0 = time.perf_counter()
    cols = np.empty((n, anchors), np.float32)
    for s0 in range(0, n, step):
        p = rx.psame(V, s0, min(step, n - s0))  # (the whole matrix crosses PCIe; only the timed anchors' columns are kept)
        cols[s0:s0 + len(p)] = p[:, :anchors]
    t_matrix = time.perf_counter() - t0
    t0 = time.perf_counter()
    out = []
    for g in range(anchors):
        p = cols[:, g].astype(np.float64)
        fpr, tpr, _ = metrics.roc_curve(cls, p, pos_label=1)
        prec, rec, _ = metrics.precision_recall_curve(cls, p, pos_label=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            f1 = np.nan_to_num(2 * prec * rec / (prec + rec))
        out.append((metrics.auc(fpr, tpr), metrics.average_precision_score(cls, p, pos_label=1), float(f1.max())))
    return t_matrix, time.perf_counter() - t0, out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rows", default="1200000")
    ap.add_argument("--vectors", default="124,1000")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-anchors", type=int, default=8)
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
    say(f"# per-anchor ranking quality: (a) ReportIndex.psame + download + sklearn per anchor ({a.host_anchors} anchors timed, scaled to all)  vs  (b) RankIndex.rank; "
        f"{a.repeats} repeats after a warm-up, wall clock and kernel time in ms")
    beats = True
    for n in [int(x) for x in a.rows.split(",")]:
        U = embeddings(n, 512, 1)
        cls = (np.random.default_rng(3).random(n) < 0.0032).astype(np.uint8)
        with retrieve.ReportIndex(0, 512, Wm, 0) as rx, rank.RankIndex(0, 512, Wm, 0) as kx:
            t0 = time.perf_counter()
            for s0 in range(0, n, 65536):
                kx.add(U[s0:s0 + 65536])
            kx.set_classes(cls)
            say(f"N={n}: fill of the ranking index (add from host memory, 65536 rows per call, and the classes) {1e3 * (time.perf_counter() - t0):.1f} ms")
            for s0 in range(0, n, 65536):
                rx.add(U[s0:s0 + 65536])
            for G in [int(x) for x in a.vectors.split(",")]:
                V = embeddings(G, 512, 2)
                kx.rank(V, bank=True)  # the warm-up: first launches load code objects, the workspace grows
                wall, stages = [], []
                for _ in range(a.repeats):
                    t0 = time.perf_counter()
                    got = kx.rank(V, bank=True)
                    wall.append(1e3 * (time.perf_counter() - t0))
                    stages.append(kx.stage_ms())
                med = {k: float(np.median([s[k] for s in stages])) for k in stages[0]}
                bound = max(("score", "sort", "statistics"), key=lambda k: med[k])
                walls, kernels = " ".join(f"{t:.1f}" for t in wall), " ".join(f"{s['total']:.1f}" for s in stages)
                say(f"N={n} G={G} (b) rank with the bank slot: wall {walls}  kernels {kernels}  median stages: score {med['score']:.1f}  sort {med['sort']:.1f}  "
                    f"statistics {med['statistics']:.1f}  -> {n * G / (med['total'] * 1e-3):.3g} rows x vectors / s of kernel time; the {bound} stage bounds the call "
                    f"({100 * med[bound] / med['total']:.0f} % of the kernel time)")
                k = min(a.host_anchors, G)
                t_matrix, t_sk, ref = host_route(rx, V, n, cls, k)
                scaled = 1e3 * (t_matrix + t_sk * G / k)
                close = all(x is not None and abs(x - r[0]) <= 1e-12 for x, r in zip(got["auc"][:k], ref)) and all(abs(float(x) - r[1]) <= 1e-12 for x, r in zip(got["ap"][:k], ref))
                f1 = [2 * tp / (tp + fp + npos) for (tp, fp), npos in zip(got["best"][:k].tolist(), got["n"][:k, 1].tolist())]
                close = close and all(abs(x - r[2]) <= 1e-12 for x, r in zip(f1, ref))
                faster = scaled > max(wall)
                beats = beats and faster and close
                say(f"N={n} G={G} (a) the matrix to the host {1e3 * t_matrix:.0f} ms (measured in full) + sklearn {1e3 * t_sk / k:.0f} ms per anchor (measured on {k}, SCALED to {G}) "
                    f"= {scaled:.0f} ms  ratio to (b)'s median wall {scaled / np.median(wall):.0f}x  AUC, AP and best F1 of the {k} anchors agree to 1e-12: {close}  (b) faster: {faster}")
    say(f"the device route beats the host route at every shape, with equal figures: {'PASS' if beats else 'FAIL'}")
    return 0 if beats else 1


if __name__ == "__main__":
    sys.exit(main())
