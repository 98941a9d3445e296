"""What the sink census costs at the bench shape (GPU): batches of 256 issue reports of 256 tokens, bert-base geometry, 12 layers, the
resident sweep on two streams as bench.py runs it (synth.make_weights default weights, MV_F16X8 in the default form, a synthetic bank of 128 anchors).

Runs ALTERNATE between the settings, each in a fresh child process on the same build: census off, census on and — with --parent-root, the tree of the parent
commit with its library built — the parent commit's code (which has no census).  Every child warms up, times --repeat sweeps of --rows rows (issue reports/s
each) and, in the census settings, sweeps once more on one stream with HIP events on the kernel class the census launches are recorded under ("attention":
mv_profile_select): the census-on run has 11 launches more per pass, and (ms_on - ms_off) / (launches_on - launches_off) is the event time per census launch.
Nothing is asserted: the figures are written down (--out, default profiles/sink_census_bench.txt).
Usage: python scripts/sink_census_rate.py [--rounds 3] [--repeat 3] [--rows 4096] [--parent-root DIR] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, S, G = 256, 256, 128


def child(mode, root, rows, repeat):
    sys.path.insert(0, root)
    import numpy as np  # noqa: F401
    from memvul_amd import synth
    from memvul_amd.binding import Engine

    dims = synth.BertDims()
    eng = Engine(0, vocab_size=dims.vocab_size, layers=dims.layers, max_tokens=max(B * S, 128 * 512), max_batch=B, max_anchors=1024)
    eng.load_state_dict(synth.make_weights(dims), "precise")
    if mode == "on":
        eng.sink_census_enable(True)
    eng.anchor_set(synth.make_anchor_bank(G))
    ids, lens = synth.make_ids(rows, S, dims.vocab_size, seed=synth.SEED + 1000)
    eng.corpus_upload(ids, lens)
    out = {"mode": mode, "rates": []}
    for it in range(repeat + 1):  # (the first sweep warms up)
        eng.sync()
        t0 = time.perf_counter()
        eng.corpus_run(0, rows, B)
        eng.sync()
        t = time.perf_counter() - t0
        if it:
            out["rates"].append(rows / t)
    if mode != "parent":
        eng.set_streams(1)  # (one batch in flight: an event span then belongs to its own launch)
        eng.profile_select(["attention"])
        eng.profile_enable(True)
        eng.corpus_run(0, rows, B)
        ms, n = eng.profile_read()["attention"]
        eng.profile_enable(False)
        out.update(attention_ms=ms, attention_launches=n)
    if mode == "on":
        c = eng.sink_census(top=3)
        out.update(flagged_items=c["flagged_items"], top=[(r["token_id"], r["items"]) for r in c["tokens"]])
    eng.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--parent-root", default=None, help="a tree of the parent commit with its library built: its rate is measured in the same alternation")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sink_census_bench.txt"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.root, args.rows, args.repeat)
    modes = (["parent"] if args.parent_root else []) + ["off", "on"]
    runs = {m: [] for m in modes}
    lines = ["sink census at the bench shape: batches of %d x %d tokens, 12 layers, MV_F16X8 default form, %d rows per sweep, two streams" % (B, S, args.rows),
             "%d rounds alternating %s; %d timed sweeps per run (issue reports/s each)" % (args.rounds, " / ".join(modes), args.repeat)]
    for r in range(args.rounds):
        for m in modes:
            root = args.parent_root if m == "parent" else ROOT
            cmd = [sys.executable, os.path.abspath(__file__), "--child", m, "--root", root, "--rows", str(args.rows), "--repeat", str(args.repeat)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            res = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not res:
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit("run %d of %r failed (exit %d): nothing more is started" % (r, m, p.returncode))
            out = json.loads(res[-1][7:])
            runs[m].append(out)
            lines.append("round %d %-6s %s" % (r, m, " ".join("%.0f" % x for x in out["rates"])))
            print(lines[-1], flush=True)
    lines.append("")
    best = {}
    for m in modes:
        allr = [x for o in runs[m] for x in o["rates"]]
        per_run = [max(o["rates"]) for o in runs[m]]
        best[m] = max(allr)
        lines.append("%-6s best %.0f, median %.0f, best of each run %s (spread %.2f %% of the best)"
                     % (m, max(allr), sorted(allr)[len(allr) // 2], " ".join("%.0f" % x for x in per_run), 100 * (max(per_run) - min(per_run)) / max(per_run)))
    lines.append("census on / off (best): %.4f" % (best["on"] / best["off"]))
    if "parent" in best:
        lines.append("census off / parent commit (best): %.4f" % (best["off"] / best["parent"]))
    on, off = runs["on"][-1], runs["off"][-1]
    dn = on["attention_launches"] - off["attention_launches"]
    per = [(a["attention_ms"] - b["attention_ms"]) / (a["attention_launches"] - b["attention_launches"]) * 1e3 for a, b in zip(runs["on"], runs["off"])]
    lines.append("HIP events, class 'attention', one sweep on one stream: off %.3f ms in %d launches, on %.3f ms in %d launches"
                 % (off["attention_ms"], off["attention_launches"], on["attention_ms"], on["attention_launches"]))
    lines.append("event time per census launch (%d launches more per sweep): %s us per round; K bytes read per launch %.1f MB"
                 % (dn, " ".join("%.1f" % x for x in per), B * 12 * S * 128 / 1e6))
    lines.append("census of the bench model's sweeps (diffuse attention): flagged items %d, top %s" % (on.get("flagged_items", 0), on.get("top")))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
