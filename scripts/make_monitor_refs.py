"""CPU references for the attention kernel's CONCENTRATION MONITOR (memvul_amd/csrc/attention_v2.h, AttnArgs::conc / seq_over; tests/test_monitor_parity_gpu.py):
the float64 collision mass of the [CLS] row on the ordinary keys (oracle/concentration.py), per (layer, sequence, head), on a GRADED fixture — items on both
sides of the 0.25 threshold, at every padded width the planner produces, with the sink token moved through the sequence.

Models: the trained-like family at 3 layers, vocabulary 2048 (weights by seed; only the calibrated sink gains are stored):
  mid_cls_40 / _50 / _52   an ordinary-token sink of the [CLS] row at a mean target mass of 0.4 / 0.5 / 0.52 (0.25 ~ 0.5^2): the GRADED cases
  mid_all_50               the same sink for every row
  sep_cls_80, cls_all_80   the excluded-key controls: 80 % of the mass on [SEP] / on [CLS]; the collision mass on ORDINARY keys stays small
Sequences, per width W in 64, 128, 192, 256, 384, 512: 8 rows of W, W - 1, (previous width) + 1, 15, 16, 17 tokens and two (W = 64: three) lengths drawn in
between.  Every other occurrence of synth.MID_ID is cleared, then the sink token is written at ONE position per row: 1 (the first ordinary token), len - 2 (the
last), len // 2, nowhere ("none": an unmarked row), and for W = 384 / 512 one position inside every 128-key chunk (so that the running maximum of the chunked
kernels rises after chunk 0); row i of model k takes kind (i + k) mod the number of kinds, so every kind meets every length over the models.

Stored per (model, width): the exact float64 collision array [3, 8, 12], the shipped-default rounding model's and the safe form's model array.  `delta_abs` =
3 x the largest |model - exact| over every monitored item of the fixture; the band of an item is delta_abs + 2^-10 x its collision mass (the recording format
stands in the place of P's fp16 rounding, and the kernel squares fp16 probabilities).  The reference is the exact array; the models only size the margin.
The conditions the GPU test relies on are asserted here on the reference alone (check()).
Usage: python scripts/make_monitor_refs.py [--jobs N] [--check]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from memvul_amd import synth  # noqa: E402
from oracle import concentration as conc  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "monitor_refs.npz")
DIMS = dict(layers=3, vocab_size=2048)
KW = dict(qk_scale=2.0, match_scale=29.0, trained_like=True)
WIDTHS = (64, 128, 192, 256, 384, 512)
# name -> (token, rows, target, seed, graded)
MODELS = {
    "mid_cls_40": ("mid", "cls", 0.4, 5001, True),
    "mid_cls_50": ("mid", "cls", 0.5, 5002, True),
    "mid_cls_52": ("mid", "cls", 0.52, 5003, True),  # (0.55 and 0.6 put more than 80 % of the items of the 384-token case over the threshold)
    "mid_all_50": ("mid", "all", 0.5, 5014, False),  # (seed 5004: the calibration of layers 1 and 2 does not converge)
    "sep_cls_80": ("sep", "cls", 0.8, 5005, False),
    "cls_all_80": ("cls", "all", 0.8, 5006, False),
}
FORMS = ("shipped", "safe")
# whole batches (tests/test_gpu_kernels.py test_attention_persistent_item_loop's list) on BATCH_MODEL, every other row marked; and the mixed batches of
# tests/golden/guarded_form_refs.npz (12 layers: the 11 monitored ones are stored), whose clean rows sit at the per-sequence rule's edge
BATCHES = ((48, 256), (70, 128), (40, 192), (26, 512), (30, 384), (21, 320))
BATCH_MODEL = "mid_cls_50"
GUARDED_CASES = ("mid_all_80_3001", "mid_all_50_3002", "mid_cls_80_3003")
P_ROUNDING = 2.0 ** -10  # relative: two fp16 roundings of p (2 x 2^-11), squared probabilities


def dims():
    return synth.BertDims(**DIMS)


def weights(name, gains):
    token, rows, _, seed, _ = MODELS[name]
    return synth.make_weights(dims(), seed=seed, sink=dict(token=token, rows=rows, gains=list(gains)), **KW)


def calibrate(name):
    token, rows, target, seed, _ = MODELS[name]
    gains = np.asarray(synth.calibrate_sink(dims(), seed, target, token, rows, n=3, **KW), np.float32)
    assert gains.max() < 8.0, (name, gains)  # (the bisection's upper end is 64: a draw whose calibration does not converge is not a model of anything)
    return gains


def kinds(W):
    """The sink positions of width W in the order the rows of a case cycle through (the last chunks early: they need the longest rows, which come first)."""
    return ["first", "last", "half"] + ["chunk%d" % c for c in reversed(range(W // 128 if W > 256 else 0))] + ["none"]


def place_sink(ids, n, kind):
    """ids (one row, in place) with synth.MID_ID at the position `kind` names and nowhere else; returns the position (-1: none)."""
    ids[ids == synth.MID_ID] = synth.MID_ID + 1
    if kind.startswith("chunk"):
        pos = 128 * int(kind[5:]) + 70
        pos = pos if pos <= n - 2 else n // 2
    else:
        pos = {"first": 1, "last": n - 2, "half": n // 2, "none": -1}[kind]
    if pos >= 0:
        ids[pos] = synth.MID_ID
    return pos


def case_inputs(name, W):
    """(ids [8, W], lens [8], sink positions [8], kinds [8]) of one (model, width) case."""
    k, wi = list(MODELS).index(name), WIDTHS.index(W)
    prev = WIDTHS[wi - 1] if wi else 0
    rng = np.random.Generator(np.random.PCG64(MODELS[name][3] * 1000 + W))
    fixed = [W, W - 1] + ([prev + 1] if prev else []) + [15, 16, 17]
    lens = np.array(fixed + sorted(int(x) for x in rng.integers(max(18, prev + 2), W - 1, size=8 - len(fixed))), np.int32)
    ids, _ = synth.make_ids(8, W, DIMS["vocab_size"], seed=MODELS[name][3] + W)
    kk, pos, names = kinds(W), [], []
    for b, n in enumerate(lens):
        n = int(n)
        ids[b, n - 1], ids[b, n:] = synth.SEP_ID, 0
        names.append(kk[(b + k) % len(kk)])
        pos.append(place_sink(ids[b, :n], n, names[-1]))
    return np.ascontiguousarray(ids, np.int32), lens, np.array(pos), names


def padded(S):
    return -(-S // 64) * 64 if S <= 256 else -(-S // 128) * 128


def batch_inputs(B, S):
    """(ids [B, S], lens [B], sink positions [B]) of one whole batch: ragged, rows 2 and 3 of 15 and 16 tokens, the even rows marked at moving positions."""
    ids, lens = synth.make_ids(B, S, DIMS["vocab_size"], seed=6000 + S, ragged=True, min_len=12)
    lens[2:4] = (15, 16)
    kk = [k for k in kinds(padded(S)) if k != "none"]
    pos = []
    for b, n in enumerate(lens):
        n = int(n)
        ids[b, n - 1], ids[b, n:] = synth.SEP_ID, 0
        pos.append(place_sink(ids[b, :n], n, kk[(b // 2) % len(kk)] if b % 2 == 0 else "none"))
    return np.ascontiguousarray(ids, np.int32), lens, np.array(pos)


def guarded_inputs(case):
    """scripts/make_guarded_form_refs.py mixed_case: (dims, weights, ids [16, 256], lens, aids [12, 512], alens, marked rows, marked anchors)."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import make_guarded_form_refs as mg

    return mg.mixed_case(case, np.load(mg.SINK_REFS))


def compute_batches(gains):
    w, out = weights(BATCH_MODEL, gains), {}
    for B, S in BATCHES:
        ids, lens, _ = batch_inputs(B, S)
        out["batch_%d_%d_exact" % (B, S)] = conc.cls_collision(w, ids, lens)
        print("batch %d x %d done" % (B, S), flush=True)
    return out


def compute_guarded(case):
    _, w, ids, lens, aids, alens, _, _ = guarded_inputs(case)
    LA = int(alens.max())
    ex = np.concatenate([conc.cls_collision(w, ids, lens), conc.cls_collision(w, aids[:, :LA], alens)], 1)  # [12, 16 + 12, 12]
    print("guarded case %s done" % case, flush=True)
    return {"guarded_%s_exact" % case: ex[:-1]}


def model_cfg(form, layers=DIMS["layers"]):
    """(cfg, encode keyword arguments) of the rounding model of a form: tests/test_guarded_form_cpu.py's `default` and `safe`."""
    from oracle import precision_model as pm

    if form == "shipped":
        return pm.engine_formats(layers, "f16", **pm.X8_ENGINE_SHIPPED), dict(pm.SHIPPED_KW)
    return pm.engine_formats(layers, "f16", **dict(pm.X8_ENGINE, a_qkv="f16x8", qkv="f16x2", p="f16x2")), {}


def compute_model(name):
    out = {name + "_gains": calibrate(name)}
    w = weights(name, out[name + "_gains"])
    for W in WIDTHS:
        ids, lens, _, _ = case_inputs(name, W)
        out["%s_%d_exact" % (name, W)] = conc.cls_collision(w, ids, lens)
        for form in FORMS:
            cfg, kw = model_cfg(form)
            out["%s_%d_%s" % (name, W, form)] = conc.cls_collision(w, ids, lens, cfg, **kw)
        print("%s width %d done" % (name, W), flush=True)
    return out


def band(coll, delta_abs):
    return delta_abs + P_ROUNDING * coll


def verdicts(exact, lens, delta_abs, layers):
    """Per sequence over the first `layers` layers: (low, high) = the fewest / the most items over the threshold that the band allows, and the rule's verdict
    on each (equal: no band item can change it)."""
    e = exact[:layers] * (np.asarray(lens) >= conc.MIN_LEN)[None, :, None]
    lo = (e > conc.THRESHOLD + band(e, delta_abs)).sum(axis=(0, 2))
    hi = (e > conc.THRESHOLD - band(e, delta_abs)).sum(axis=(0, 2))
    return lo, hi, conc.rule(lo, lens, layers), conc.rule(hi, lens, layers)


def check(refs, verbose=True):
    """delta_abs from the stored arrays, and the conditions on the reference alone; returns delta_abs."""
    say = print if verbose else (lambda *a, **k: None)
    gap = {}
    for name in MODELS:
        for W in WIDTHS:
            lens = case_inputs(name, W)[1]
            mon = lens >= conc.MIN_LEN
            ex = refs["%s_%d_exact" % (name, W)]
            gap[name, W] = {f: float(np.abs(refs["%s_%d_%s" % (name, W, f)] - ex)[:, mon].max()) for f in FORMS}
    delta_abs = 3.0 * max(max(g.values()) for g in gap.values())
    say("delta_abs = 3 x %.3e = %.3e (+ 2^-10 x collision: %.3e at the threshold)" % (delta_abs / 3, delta_abs, band(conc.THRESHOLD, delta_abs)))
    L = DIMS["layers"]
    seen = {W: set() for W in WIDTHS}
    graded_rows = graded_clear = 0
    for name, (_, _, _, _, graded) in MODELS.items():
        for W in WIDTHS:
            lens = case_inputs(name, W)[1]
            mon = lens >= conc.MIN_LEN
            ex = refs["%s_%d_exact" % (name, W)][:, mon]
            near = float((np.abs(ex - conc.THRESHOLD) <= band(ex, delta_abs)).mean())
            over = float((ex > conc.THRESHOLD).mean())
            clear = np.ones(len(lens), bool)
            for layers in (L - 1, L):
                lo, hi, v_lo, v_hi = verdicts(refs["%s_%d_exact" % (name, W)], lens, delta_abs, layers)
                clear &= v_lo == v_hi
                seen[W] |= set(v_lo[(v_lo == v_hi) & mon].tolist())
            say("%s width %3d: max |model - exact| shipped %.2e safe %.2e; items over %.0f %%, within the band %.1f %%, max %.3f; rows with a clear verdict %d of 8"
                % (name, W, gap[name, W]["shipped"], gap[name, W]["safe"], 100 * over, 100 * near, float(ex.max()), int(clear.sum())))
            assert near <= 0.05, (name, W, near)
            if graded:
                assert over >= 0.2 and 1 - over >= 0.2, (name, W, over)
                graded_rows += len(lens)
                graded_clear += int(clear.sum())
    assert 4 * graded_clear >= graded_rows, (graded_clear, graded_rows)
    assert all(s == {True, False} for s in seen.values()), seen
    say("graded rows with a verdict no band item can change: %d of %d; both verdicts occur at every width" % (graded_clear, graded_rows))
    return delta_abs


def compute(job):
    """One job of the fixture: a model's six widths, a guarded-form case, or (given the gains of BATCH_MODEL) the whole batches."""
    if job in MODELS:
        return compute_model(job)
    if job.startswith("guarded_"):
        return compute_guarded(job[len("guarded_"):])
    return compute_batches(calibrate(BATCH_MODEL))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=1)
    ap.add_argument("--check", action="store_true", help="only re-check the committed fixture")
    ap.add_argument("--only", nargs="*", help="compute these jobs alone and merge them into the fixture (a model name, guarded_<case>, batches)")
    args = ap.parse_args()
    if args.check:
        check(np.load(OUT))
        return
    jobs = args.only or (["guarded_" + c for c in GUARDED_CASES] + ["batches"] + list(MODELS))  # (the longest first)
    if args.jobs > 1:
        import multiprocessing as mp

        with mp.get_context("spawn").Pool(args.jobs) as pool:
            parts = pool.map(compute, jobs, chunksize=1)
    else:
        parts = [compute(j) for j in jobs]
    have = dict(np.load(OUT)) if args.only and os.path.exists(OUT) else {}
    for p in parts:
        have.update(p)
    have.pop("delta_abs", None)
    np.savez_compressed(OUT, **have)  # (first without delta_abs: a draw that misses a condition can be looked at with --check; the tests refuse such a file)
    have["delta_abs"] = np.float64(check(have))
    np.savez_compressed(OUT, **have)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
