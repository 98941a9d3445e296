"""CPU references for the SINK CENSUS (memvul_amd/csrc/sink_census.h; tests/test_sink_census_gpu.py, tests/test_sink_census_cpu.py): per (layer, sequence, head)
item the float64 collision mass of the [CLS] row on the ordinary keys, the token position with the largest ordinary share, that share, the runner-up's position
and share and the third share (tests/census_kit.py summarise, on probabilities read as oracle/concentration.py reads them).

Models: the trained-like family at 3 layers, vocabulary 30522 (weights by seed; only the calibrated sink gains are stored):
  ord_40 / ord_50 / ord_80   an ordinary-token sink (synth.MID_ID) of the [CLS] row at a mean target mass of 0.4 / 0.5 / 0.8 (the vocabulary is bert-base's
                             30522 ids: with the monitor fixture's 2048 the random ids of synth.calibrate_sink's own sequences repeat the sink token often
                             enough that the mass at ITS position cannot reach 0.7, and the bisection runs into its upper end)
  two_tok                    ord_80's construction plus a SECOND sink token (SECOND_ID) whose flag in the embedding is SECOND_FLAG x the first one's: two
                             different sink tokens of different strength
  ctl_sep_80, ctl_cls_80     the controls: 80 % of the mass on [SEP] / on [CLS]; nothing on the ordinary keys goes over the threshold
Sequences, per padded width W in 64 (the two-plane short pass), 192 (a tile spans two sequences), 256, 512 (the chunked attention): 8 rows of W, W - 1, 17, 16,
15, W and two drawn lengths.  Every occurrence of the sink tokens is cleared, then the sink token is written by the row's KIND: at position 1 (the engine's
last row), len - 2, len // 2, inside each 128-key chunk, TWICE (len // 3 and 2 len // 3: the first occurrence wins only where its share is larger), nowhere.
Row i of model k takes kind (i + k) mod the number of kinds.  In two_tok the second token goes to position (len // 2) + 3 of every row.

Uncertain items: collision mass inside the monitor suite's band around 0.25 (delta_abs of tests/golden/monitor_refs.npz + 2^-10 x the mass), or top and
runner-up shares of DIFFERENT tokens closer than m = 3 x the largest |rounding-model p - exact p| over the ordinary keys of the monitored rows of the fixture
(precision_model in the shipped default's formats; never a GPU value).  check() asserts on the float64 reference alone that they are
at most 5 % of the possibly-over items of every case, that no third share comes within m of the top one, and that the cases hold what the tests rely on.
Usage: python scripts/make_sink_census_refs.py [--jobs N] [--check]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from memvul_amd import synth  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "sink_census_refs.npz")
MONITOR_REFS = os.path.join(ROOT, "tests", "golden", "monitor_refs.npz")
DIMS = dict(layers=3, vocab_size=30522)
KW = dict(qk_scale=2.0, match_scale=29.0, trained_like=True)
WIDTHS = (64, 192, 256, 512)
SECOND_ID, SECOND_FLAG = 1500, 0.8
# name -> (token, rows, target, seed, control)
MODELS = {
    "ord_40": ("mid", "cls", 0.4, 5001, False),
    "ord_50": ("mid", "cls", 0.5, 5002, False),
    "ord_80": ("mid", "cls", 0.8, 5021, False),
    "two_tok": ("mid", "cls", 0.8, 5022, False),
    "ctl_sep_80": ("sep", "cls", 0.8, 5037, True),  # (seeds 5005 / 5015: one head of one drawn row sits on an ordinary token by itself, collision mass 0.31 — no control)
    "ctl_cls_80": ("cls", "all", 0.8, 5006, True),
}
FORMS = ("shipped",)  # the rounding model that sizes m: the shipped default's formats
KEYS = ("coll", "pos1", "share1", "pos2", "share2", "share3")
VOCAB_WORDS = {synth.MID_ID: ".", SECOND_ID: "##ing", synth.CLS_ID: "[CLS]", synth.SEP_ID: "[SEP]"}  # the fixture's vocabulary strings (the rest: "tok<id>")


def dims():
    return synth.BertDims(**DIMS)


def weights(name, gains):
    token, rows, _, seed, _ = MODELS[name]
    w = synth.make_weights(dims(), seed=seed, sink=dict(token=token, rows=rows, gains=list(gains)), **KW)
    if name == "two_tok":
        k = synth.PFX_BERT + "embeddings.word_embeddings.weight"
        w[k] = w[k].copy()
        w[k][SECOND_ID, synth.SINK_DIM] += np.float32(SECOND_FLAG * synth.SINK_FLAG)
    return w


def calibrate(name):
    token, rows, target, seed, _ = MODELS[name]
    gains = np.asarray(synth.calibrate_sink(dims(), seed, target, token, rows, n=3, **KW), np.float32)
    assert gains.max() < 8.0, (name, gains)  # (a draw whose calibration does not converge is not a model of anything)
    return gains


def kinds(W):
    return ["first", "last", "half"] + ["chunk%d" % c for c in reversed(range(-(-W // 128) if W > 128 else 0))] + ["twice", "none"]


def place_sink(ids, n, kind):
    """ids (one row, in place) with synth.MID_ID where `kind` says and nowhere else; returns its positions."""
    for t in (synth.MID_ID, SECOND_ID):
        ids[ids == t] = t + 1
    if kind.startswith("chunk"):
        pos = 128 * int(kind[5:]) + 40
        pos = [pos if pos <= n - 2 else n // 2]
    else:
        pos = {"first": [1], "last": [n - 2], "half": [n // 2], "twice": [n // 3, 2 * n // 3], "none": []}[kind]
    for p in pos:
        ids[p] = synth.MID_ID
    return pos


def case_inputs(name, W):
    """(ids [8, W], lens [8], kinds [8]) of one (model, width) case."""
    k = list(MODELS).index(name)
    rng = np.random.Generator(np.random.PCG64(MODELS[name][3] * 1000 + W))
    lens = np.array([W, W - 1, 17, 16, 15, W] + sorted(int(x) for x in rng.integers(18, W - 1, size=2)), np.int32)
    ids, _ = synth.make_ids(8, W, DIMS["vocab_size"], seed=MODELS[name][3] + W)
    kk, names = kinds(W), []
    for b, n in enumerate(lens):
        n = int(n)
        ids[b, n - 1], ids[b, n:] = synth.SEP_ID, 0
        names.append(kk[(b + k) % len(kk)])
        taken = place_sink(ids[b, :n], n, names[-1])
        if name == "two_tok" and n // 2 + 3 <= n - 2 and n // 2 + 3 not in taken:
            ids[b, n // 2 + 3] = SECOND_ID
    return np.ascontiguousarray(ids, np.int32), lens, names


def model_cfg(form, layers=DIMS["layers"]):
    from oracle import precision_model as pm

    if form == "shipped":
        return pm.engine_formats(layers, "f16", **pm.X8_ENGINE_SHIPPED), dict(pm.SHIPPED_KW)
    return pm.engine_formats(layers, "f16", **dict(pm.X8_ENGINE, a_qkv="f16x8", qkv="f16x2", p="f16x2")), {}


def compute_gains(name):
    return {name + "_gains": calibrate(name), name + "_seed": np.int64(MODELS[name][3])}


def compute_case(job):
    """One (model, width) case: the exact rows' summary, the largest |rounding-model p - exact p| over the ordinary keys of its monitored rows, its inputs."""
    import census_kit as ck

    name, W, gains = job
    out = {}
    w = weights(name, gains)
    ids, lens, _ = case_inputs(name, W)
    p = ck.cls_rows(w, ids, lens)
    for k, v in ck.summarise(p, lens).items():
        out["%s_%d_%s" % (name, W, k)] = v
    gap = 0.0
    for form in FORMS:
        cfg, kw = model_cfg(form)
        pmod = ck.cls_rows(w, ids, lens, cfg, **kw)
        for b, n in enumerate(lens):
            if n >= ck.MIN_LEN:
                gap = max(gap, float(np.abs(pmod[:, b, :, 1:int(n) - 1] - p[:, b, :, 1:int(n) - 1]).max()))
    out["%s_%d_pgap" % (name, W)] = np.float64(gap)
    out["%s_%d_ids" % (name, W)], out["%s_%d_lens" % (name, W)] = ids, lens
    print("%s width %d done (largest |model p - exact p| %.3e)" % (name, W, gap), flush=True)
    return out


def case_ref(refs, name, W):
    return {k: refs["%s_%d_%s" % (name, W, k)] for k in KEYS}


def check(refs, verbose=True):
    """m and the conditions on the reference alone; returns m."""
    import census_kit as ck

    say = print if verbose else (lambda *a, **k: None)
    delta_abs = float(np.load(MONITOR_REFS)["delta_abs"])
    m = 3.0 * max(float(refs["%s_%d_pgap" % (n, W)]) for n in MODELS for W in WIDTHS)
    say("delta_abs = %.3e (monitor suite), m = 3 x %.3e = %.3e" % (delta_abs, m / 3, m))
    seen_kinds = set()
    for name, (_, _, _, _, control) in MODELS.items():
        tokens = set()
        for W in WIDTHS:
            ids, lens, names = case_inputs(name, W)
            assert np.array_equal(ids, refs["%s_%d_ids" % (name, W)]) and np.array_equal(lens, refs["%s_%d_lens" % (name, W)]), (name, W)
            for layers in (2, 3):
                bd = ck.bounds(case_ref(refs, name, W), ids, lens, layers, DIMS["vocab_size"], delta_abs, m)  # (asserts the third-share condition)
                assert bd["uncertain"] <= 0.05 * max(bd["possible"], 1), (name, W, layers, bd["uncertain"], bd["possible"])
                if control:
                    assert bd["possible"] == 0, (name, W, bd["possible"])
            tokens |= set(np.flatnonzero(bd["lo"]).tolist())
            over16 = bd["possible"] and (case_ref(refs, name, W)["coll"][:, 3] > ck.T).any()
            say("%s width %3d: possibly over %d, uncertain %d, certain per token %s, the 16-token row over: %s"
                % (name, W, bd["possible"], bd["uncertain"], {int(t): int(bd["lo"][t]) for t in np.flatnonzero(bd["lo"])}, bool(over16)))
            if not control:
                for b, kd in enumerate(names):
                    if lens[b] >= ck.MIN_LEN and (case_ref(refs, name, W)["coll"][:, b] > ck.T + ck.band(ck.T, delta_abs)).any():
                        seen_kinds.add(kd if not kd.startswith("chunk") else "chunk")
        if not control:
            assert synth.MID_ID in tokens, (name, tokens)
        if name == "two_tok":
            assert SECOND_ID in tokens, tokens
    assert seen_kinds >= {"first", "last", "half", "chunk", "twice"}, seen_kinds
    say("kinds with a certain item over the threshold: %s" % sorted(seen_kinds))
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=1)
    ap.add_argument("--check", action="store_true", help="only re-check the committed fixture")
    args = ap.parse_args()
    if args.check:
        check(np.load(OUT))
        return
    import multiprocessing as mp

    have = {}
    with mp.get_context("spawn").Pool(max(args.jobs, 1)) as pool:
        for part in pool.map(compute_gains, list(MODELS), chunksize=1):
            have.update(part)
        print({n: have[n + "_gains"].tolist() for n in MODELS}, flush=True)
        jobs = [(n, W, have[n + "_gains"]) for W in reversed(WIDTHS) for n in MODELS]  # (the longest first)
        for part in pool.imap_unordered(compute_case, jobs, chunksize=1):
            have.update(part)
    np.savez_compressed(OUT + ".tmp.npz", **have)  # (kept when a condition fails, so that the draw can be looked at)
    have["m"] = np.float64(check(have))
    np.savez_compressed(OUT, **have)
    os.remove(OUT + ".tmp.npz")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
